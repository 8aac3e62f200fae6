/*
 * hipfeat.h -- C ABI of libhipfeat.so: batched Kaldi-style audio feature extraction
 * (spectrogram / log-spectrogram / log-mel filterbank / MFCC) on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of lhotse: the arithmetic behind
 *   FeatureExtractor.extract / extract_batch   (lhotse/features/base.py:75-82, :152-222)
 * as implemented by the torch layers
 *   Wav2Win -> Wav2FFT -> Wav2Spec / Wav2LogSpec / Wav2LogFilterBank / Wav2MFCC
 *                                              (lhotse/features/kaldi/layers.py:59-724)
 * and driven by _extract_batch                 (lhotse/features/kaldi/extractors.py:485-554).
 *
 * The reference has no native code and therefore no FFI for this path; its FFI
 * convention elsewhere is ctypes.CDLL + integer status codes
 * (lhotse/tools/libsox.py:74-117).  Every entry point below is plain C: opaque
 * handles, raw pointers, sizes; no torch / Python types.  It is loadable with
 * ctypes or cffi (see INTEGRATION.md for the binding a lhotse maintainer would add).
 *
 * Conventions
 *   - every function returns hipfeat_status (0 == OK) unless stated otherwise;
 *     hipfeat_last_error() returns a thread-local message for the last failure;
 *   - "d_" pointers are device (HBM) pointers on the plan's device, "h_" pointers are host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued asynchronously on it, nothing synchronises the device;
 *   - no global state; safe to call with the Python GIL released; a plan may be used
 *     from several host threads as long as they use different streams.
 */
#ifndef HIPFEAT_H_
#define HIPFEAT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPFEAT_ABI_VERSION 8

#if defined(HIPFEAT_BUILD)
#define HIPFEAT_API __attribute__((visibility("default")))
#else
#define HIPFEAT_API
#endif
/* Entry points added to an ABI version WITHOUT a bump carry their own export macro, so that the set the version number stands for can
 * still be told from what was added to it (lhotse_amd/_lib.py: _LEVEL_SIGNATURES, _COLLATE_SIGNATURES, _SINC_SIGNATURES,
 * _FEATMIX_SIGNATURES, _STATS_SIGNATURES, _STFT_SIGNATURES, _CHANNELS_SIGNATURES and _REVERB_FFT_SIGNATURES next to _SIGNATURES). */
#define HIPFEAT_COLLATE_API HIPFEAT_API
#define HIPFEAT_FEATMIX_API HIPFEAT_API
#define HIPFEAT_LEVEL_API HIPFEAT_API
#define HIPFEAT_SINC_API HIPFEAT_API
#define HIPFEAT_STATS_API HIPFEAT_API
#define HIPFEAT_STFT_API HIPFEAT_API
#define HIPFEAT_STREAM_API HIPFEAT_API
#define HIPFEAT_GRAD_API HIPFEAT_API
#define HIPFEAT_CHANNELS_API HIPFEAT_API
#define HIPFEAT_REVERB_FFT_API HIPFEAT_API
#define HIPFEAT_RAGGED_API HIPFEAT_API /* the per-row-length forms inside the stft and grad blocks (_RAGGED_SIGNATURES) */

typedef enum hipfeat_status {
  HIPFEAT_OK = 0,
  HIPFEAT_ERR_INVALID = 1,     /* bad argument / inconsistent config                        */
  HIPFEAT_ERR_HIP = 2,         /* a HIP runtime call failed (message has the hipError name) */
  HIPFEAT_ERR_UNSUPPORTED = 3, /* valid in the reference but not implemented here           */
  HIPFEAT_ERR_TOO_SHORT = 4    /* waveform shorter than the reflect padding needs; the
                                  reference raises here too (layers.py:759-764)             */
} hipfeat_status;

/* Which layer of lhotse/features/kaldi/layers.py the plan reproduces. */
typedef enum hipfeat_kind {
  HIPFEAT_SPECTROGRAM = 0,     /* Wav2Spec            layers.py:336-402 */
  HIPFEAT_LOG_SPECTROGRAM = 1, /* Wav2LogSpec         layers.py:405-473 */
  HIPFEAT_FBANK = 2,           /* Wav2LogFilterBank   layers.py:476-578 */
  HIPFEAT_MFCC = 3,            /* Wav2MFCC            layers.py:581-724 */
  /* "next" row: Whisper log-mel, log_mel_spectrogram lhotse/features/whisper_fbank.py:17-85.
   * Implies: centred frames (frame t covers samples [t*shift - N/2, t*shift + N/2), torch.stft(center=True)),
   * "reflect" edges without repeating the edge sample, fft_length == frame_length (any size, direct DFT),
   * S / shift computed frames, log10(max(mel, mel_floor)) clamped to (per-cut max - 8), then (x + 4) / 4,
   * and (S + shift/2) / shift output rows, the extra one (if any) all zeros.  window / mel as for HIPFEAT_FBANK.
   * MEMORY-MODEL NOTE (gfx950 only, by construction of this library): the per-cut clamp is finished by whichever workgroup of the
   * launch completes the cut last; the hand-off between workgroups uses agent-scope write-through (sc1) stores + vmcnt(0) in front
   * of a relaxed agent-scope counter increment, and sc1 loads behind it -- the ordering the gfx950 memory pipeline gives, NOT a
   * release / acquire pair of the HIP memory model (that pair costs an L2 write-back + invalidate per workgroup: 1.9 -> 12.7 ms per
   * 4000 cuts, measured in round 3).  The library is built for --offload-arch=gfx950 alone and refuses other devices at plan creation,
   * so no caller can meet this path on hardware where the assumption does not hold; a launch that faults leaves the per-cut counters
   * of its layout armed -- destroy the layout (or plan) after a HIPFEAT_ERR_HIP from a Whisper extraction instead of re-using it. */
  HIPFEAT_WHISPER = 4,
  /* librosa-style log-mel (lhotse/features/librosa_fbank.py:66-137): the arithmetic of HIPFEAT_FBANK (set use_fft_mag = 1
   * for librosa's |X|) on centred frames with "reflect" edges (librosa.stft center=True, pad_mode="reflect"), log10 instead of
   * ln, (S + shift/2) / shift rows.  window = periodic hann of fft_length samples, mel = slaney filters (caller's values). */
  HIPFEAT_LIBROSA_FBANK = 5
} hipfeat_kind;

/*
 * Scalar options.  Field meaning == the constructor arguments of the layers above
 * (layers.py:80-94, :247-261, :494-514, :599-621), already converted to samples.
 * The float32 constant arrays (window, mel matrix, DCT, lifter) are passed separately
 * to hipfeat_plan_create so that the caller -- who computes them with the reference's
 * own formulae -- owns their exact values.
 */
typedef struct hipfeat_config {
  int32_t struct_size;      /* = sizeof(hipfeat_config); ABI guard                              */
  int32_t kind;             /* hipfeat_kind                                                     */
  int32_t frame_length;     /* N  = floor(frame_length_s * sampling_rate)    layers.py:114     */
  int32_t frame_shift;      /* floor(frame_shift_s * sampling_rate)          layers.py:116     */
  int32_t fft_length;       /* next_power_of_2(N) or N                       layers.py:265     */
  int32_t num_filters;      /* M (mel bins);   0 for (log-)spectrogram                          */
  int32_t num_ceps;         /* C (MFCC only);  0 otherwise                                      */
  int32_t snip_edges;       /* layers.py:747-753                                                */
  int32_t remove_dc_offset; /* layers.py:155-157                                                */
  int32_t use_energy;       /* layers.py:575-576 (fbank: prepended column), :399-400, :470-471;
                               MFCC: log-energy replaces C0 (Kaldi; the intent of :721-722)     */
  int32_t raw_energy;       /* layers.py:161 vs :183                                            */
  int32_t use_fft_mag;      /* |X| instead of |X|^2                          layers.py:387-390 */
  int32_t apply_lifter;     /* cepstral_lifter > 0                           layers.py:717     */
  float preemph_coeff;      /* 0 disables                                    layers.py:165     */
  float energy_floor;       /* log-energy floored at log(energy_floor) if >0 layers.py:864     */
  float mel_floor;          /* eps of max(mel, eps).log() = 1.1920929e-07    layers.py:536,572 */
  float log_offset;         /* 1e-15 added before log in Wav2LogSpec         layers.py:467     */
  float dither;             /* must be 0 (layers.py:191-193 draws torch.randn: the host adds it)  */
  int32_t batch_hop;        /* round(frame_shift_s * sampling_rate): the hop with which
                               compute_num_frames_from_samples (lhotse/utils.py:424-434) counts the rows
                               item b keeps of a zero-padded batch row (padded_len given); differs from
                               frame_shift for fractional hops (12.5 ms @ 22.05 kHz: 276 vs 275).
                               0 = frame_shift                                                   */
} hipfeat_config;

typedef struct hipfeat_plan hipfeat_plan;     /* constants + kernel selection, per (device, config) */
typedef struct hipfeat_layout hipfeat_layout; /* device-resident description of one batch shape     */

/* ---- library ------------------------------------------------------------------- */
HIPFEAT_API int32_t hipfeat_abi_version(void);
HIPFEAT_API const char* hipfeat_last_error(void);
HIPFEAT_API hipfeat_status hipfeat_device_count(int32_t* count);

/* ---- pure host helpers (no GPU needed) ------------------------------------------ */
/* Frame count of one waveform: layers.py:747-753; for snip_edges == 0 it equals
 * compute_num_frames_from_samples (lhotse/utils.py:424-434), the contract that
 * validate_features asserts (lhotse/qa.py:286-311). */
HIPFEAT_API int64_t hipfeat_num_frames(int64_t num_samples, int32_t frame_length, int32_t frame_shift, int32_t snip_edges);
/* HIPFEAT_OK, or HIPFEAT_ERR_TOO_SHORT when reflect padding is impossible:
 * the reflection is taken on a row of `padded_len` samples (== num_samples for a
 * single waveform). */
HIPFEAT_API hipfeat_status hipfeat_check_length(int64_t padded_len, int32_t frame_length, int32_t frame_shift, int32_t snip_edges);

/* ---- plan ------------------------------------------------------------------------ */
/* window[frame_length]; mel[(fft_length/2+1) * num_filters] row-major (bin, filter) as in
 * Wav2LogFilterBank._fb (layers.py:553,563); dct[num_filters * num_ceps] row-major as in
 * Wav2MFCC._dct (layers.py:697-706); lifter[num_ceps] (layers.py:681-695).  Unused arrays
 * may be NULL.  All are HOST float32 arrays, copied to the device. */
HIPFEAT_API hipfeat_status hipfeat_plan_create(const hipfeat_config* cfg, const float* h_window, const float* h_mel,
                                   const float* h_dct, const float* h_lifter, int32_t device,
                                   hipfeat_plan** plan);
HIPFEAT_API hipfeat_status hipfeat_plan_destroy(hipfeat_plan* plan);
/* Columns written per frame: M (+1 with use_energy) | C | fft/2+1. */
HIPFEAT_API int32_t hipfeat_plan_feature_dim(const hipfeat_plan* plan);
/* Human-readable name of the kernel variant the plan dispatches to (e.g. "generic",
 * "fft512"); tests use it to assert that the specialised path is the one exercised. */
HIPFEAT_API const char* hipfeat_plan_kernel_name(const hipfeat_plan* plan);

/* ---- layout: the shape of a batch ------------------------------------------------ */
/*
 * A batch is `batch` cuts.  Cut b occupies h_wave_offsets[b] .. + h_num_samples[b] (in
 * float32 elements) of the waveform buffer -- this covers both the packed form
 * (offsets = prefix sums) and the padded (B, Smax) form (offsets = b * Smax).
 *
 * h_padded_len (nullable): the row length the edge reflection is taken on.
 *   NULL / == num_samples : every cut is reflected on its own, as Fbank.extract
 *                           (extractors.py:92-115) and kaldifeat do;
 *   == max(num_samples)   : reproduces _extract_batch (extractors.py:531-537): shorter
 *                           items read zeros past their end, and only
 *                           compute_num_frames_from_samples(num_samples) rows are produced.
 *
 * Output: cut b's features are written to rows h_out_rows[b] .. + num_frames(b) of a
 * row-major matrix with `out_row_stride` floats per row (>= feature_dim).  h_out_rows
 * NULL = packed back to back.  This covers the packed (sum T_b, F) form and the padded
 * (B, Tmax, F) form (out_rows = b * Tmax).
 */
HIPFEAT_API hipfeat_status hipfeat_layout_create(const hipfeat_plan* plan, int64_t batch, const int64_t* h_wave_offsets,
                                     const int64_t* h_num_samples, const int64_t* h_padded_len,
                                     const int64_t* h_out_rows, int64_t out_row_stride, void* stream,
                                     hipfeat_layout** layout);
HIPFEAT_API hipfeat_status hipfeat_layout_destroy(hipfeat_layout* layout);
HIPFEAT_API int64_t hipfeat_layout_total_frames(const hipfeat_layout* layout);
/* Writes the per-cut frame counts into h_num_frames[batch]. */
HIPFEAT_API hipfeat_status hipfeat_layout_num_frames(const hipfeat_layout* layout, int64_t* h_num_frames);

/* ---- the hot path ---------------------------------------------------------------- */
/* One asynchronous pass over the batch described by `layout`: d_wave -> d_out. */
HIPFEAT_API hipfeat_status hipfeat_extract_layout(const hipfeat_plan* plan, const hipfeat_layout* layout,
                                      const float* d_wave, float* d_out, void* stream);

/* Convenience: build a transient layout from host arrays and run it (same semantics). */
HIPFEAT_API hipfeat_status hipfeat_extract(const hipfeat_plan* plan, const float* d_wave, const int64_t* h_wave_offsets,
                               const int64_t* h_num_samples, const int64_t* h_padded_len, int64_t batch,
                               float* d_out, const int64_t* h_out_rows, int64_t out_row_stride, void* stream);

/* Host-memory form: h_wave / h_out are HOST buffers (pinned or pageable); the library
 * stages them through the device (H2D, kernel, D2H) on `stream` and waits for completion.
 * `wave_elems` / `out_elems` are the total buffer sizes in float32 elements. */
HIPFEAT_API hipfeat_status hipfeat_extract_host(const hipfeat_plan* plan, const float* h_wave, int64_t wave_elems,
                                    const int64_t* h_wave_offsets, const int64_t* h_num_samples,
                                    const int64_t* h_padded_len, int64_t batch, float* h_out,
                                    int64_t out_elems, const int64_t* h_out_rows, int64_t out_row_stride,
                                    void* stream);


/* ---- "next" row: fused collation of the output, int16 PCM input ------------------- */
/*
 * hipfeat_extract + collate_matrices(features, padding_value) in one call
 * (lhotse/dataset/input_strategies.py:458-462, lhotse/dataset/collation.py:506-535): d_out is a dense
 * (batch, rows_per_cut, feature_dim) float32 tensor; cut b's frames go to d_out[b, :T_b] and the rows
 * [T_b, rows_per_cut) are filled with pad_value (LOG_EPSILON in lhotse).  T_b is returned in h_num_frames
 * (may be NULL).  Fails if some T_b > rows_per_cut.
 */
HIPFEAT_API hipfeat_status hipfeat_extract_collated(const hipfeat_plan* plan, const float* d_wave, const int64_t* h_wave_offsets,
                                        const int64_t* h_num_samples, const int64_t* h_padded_len, int64_t batch,
                                        float* d_out, int64_t rows_per_cut, float pad_value, int64_t* h_num_frames,
                                        void* stream);
/* int16 PCM -> float32 in [-1, 1): x / 32768, exactly what the audio backends hand to the reference
 * (so features are bit-identical to the float32 path); lets the host send half the bytes over PCIe. */
HIPFEAT_API hipfeat_status hipfeat_pcm16_to_float(const int16_t* d_pcm, float* d_wave, int64_t num_samples, void* stream);
/* float32 -> IEEE binary16 (round to nearest even) on the device, in front of the device -> host copy of a feature batch that is going to
 * be STORED in half precision: the reference's default feature storage is lossy as well (lilcom, lhotse/features/io.py:981-1061,
 * features/compression.py:18-37: the fixture it ships is exact to 2^-6); binary16 keeps log-domain features (|x| < 32) to 2^-6 ... 2^-7
 * absolute and halves both the PCIe traffic and the file.  lilcom's own bit stream is third-party and not reproduced.  No plan: launches
 * on the calling thread's current device. */
HIPFEAT_API hipfeat_status hipfeat_float_to_half(const float* d_in, uint16_t* d_out, int64_t n, void* stream);

/* ---- "next" row: post-feature transforms on the collated (B, T, F) batch ------- */
/* GlobalMVN.forward: (x - means) / stds, and .inverse: x * stds + means, over `rows` rows of `feature_dim` floats
 * (lhotse/dataset/signal_transforms.py:50-60).  IEEE single operations in the reference's order: bit-identical. */
HIPFEAT_API hipfeat_status hipfeat_global_mvn(const float* d_in, float* d_out, const float* d_means, const float* d_stds, int64_t rows,
                                              int64_t feature_dim, int inverse, void* stream);
/*
 * SpecAugment._forward_single for every sequence of a batch in two launches
 * (lhotse/dataset/signal_transforms.py:173-266): d_out = clone of d_in with
 *   - every warp segment time-warped: rows [0, center) of the segment are resampled to [0, warped) and rows
 *     [center, num_frames) to [warped, num_frames) with torch's bicubic interpolation (time_warp, :338-371;
 *     F.interpolate(mode="bicubic", align_corners=False)).  `center` and `warped` are the two np.random.randint draws;
 *     segments of one sequence must not overlap (the reference applies them one after another);
 *   - every mask region set to the mean of ITS sequence (all num_frames * feature_dim values, after warping):
 *     axis 1 = frames [begin, end), axis 2 = feature bins [begin, end) (mask_along_axis_optimized, :297-335).
 * The random draws stay with the caller (the host mirror makes them with the reference's RNG calls in the reference's order).
 * Descriptors are host arrays; the call is asynchronous on `stream`.  d_in and d_out must not alias.
 * Like hipfeat_pcm16_to_float and hipfeat_global_mvn it has no plan: it launches on the calling thread's current device, which must
 * be the one that owns the buffers and the stream.
 */
typedef struct hipfeat_warp_segment {
  int32_t sequence, start, num_frames, center, warped;
} hipfeat_warp_segment;
typedef struct hipfeat_mask {
  int32_t sequence, axis, begin, end;
} hipfeat_mask;
HIPFEAT_API hipfeat_status hipfeat_specaug(const float* d_in, float* d_out, int64_t batch, int64_t num_frames, int64_t feature_dim,
                                           const hipfeat_warp_segment* h_segments, int64_t num_segments, const hipfeat_mask* h_masks,
                                           int64_t num_masks, void* stream);

/* ---- "next" row: speed perturbation = polyphase sinc resampling --------------- */
/*
 * Replaces ResampleTensor (lhotse/augmentation/resample.py:42-142, :284-315) as used by
 * Speed.__call__ (lhotse/augmentation/torchaudio.py:37-42).  `orig_freq` / `new_freq` are the
 * gcd-reduced rates; h_kernel is the float32 filter bank [new_freq][2*width + orig_freq] computed by
 * the caller with the reference's formula (resample.py:184-281), so its values are the caller's.
 */
typedef struct hipfeat_resampler hipfeat_resampler;
HIPFEAT_API hipfeat_status hipfeat_resampler_create(int32_t orig_freq, int32_t new_freq, int32_t width, const float* h_kernel,
                                        int32_t device, hipfeat_resampler** resampler);
HIPFEAT_API hipfeat_status hipfeat_resampler_destroy(hipfeat_resampler* resampler);
/*
 * ABI v8.  The kernel hipfeat_resample launches for this resampler, chosen once at creation: "resample_fast<9,10,7>" (a compile-time
 * instance: the speed ratios and 1:2, 2:1, 3:1), "resample_mfma" (many phases and an odd hop, e.g. 441:160 = 44.1 -> 16 kHz: the
 * strided convolution of lhotse/augmentation/resample.py:284-315 as a GEMM on the f32 matrix cores) or "resample_generic" (everything
 * else, and everything under HIPFEAT_RESAMPLE_GENERIC=1).  All three sum a sample's taps in ascending order; their outputs are equal.
 * The string lives as long as the resampler.
 */
HIPFEAT_API const char* hipfeat_resampler_kernel_name(const hipfeat_resampler* resampler);
/* ceil(new * num_samples / orig), evaluated like the reference (in float32, resample.py:309). */
HIPFEAT_API int64_t hipfeat_resampled_length(int64_t num_samples, int32_t orig_freq, int32_t new_freq);
/* Batch of cuts: cut b = d_in[h_in_offsets[b] .. + h_num_samples[b]) -> d_out[h_out_offsets[b] .. + resampled_length). */
HIPFEAT_API hipfeat_status hipfeat_resample(const hipfeat_resampler* resampler, const float* d_in, const int64_t* h_in_offsets,
                                const int64_t* h_num_samples, int64_t batch, float* d_out, const int64_t* h_out_offsets,
                                void* stream);

/* ---- on-the-fly mini-batch: mixed-factor speed perturbation + collated extraction in TWO launches ------------- */
/*
 * BASELINE configs[4].  What OnTheFlyFeatures does per mini-batch on the CPU -- Speed per cut inside Recording.load_audio
 * (lhotse/dataset/cut_transforms/perturb_speed.py:8-47, lhotse/augmentation/torchaudio.py:37-42, augmentation/resample.py:284-315),
 * extract_batch, collate_matrices with LOG_EPSILON (lhotse/dataset/input_strategies.py:410-462, dataset/collation.py:506-535) --
 * on a packed mini-batch that is resident in ONE device buffer (the "arena": the cuts at h_offsets / h_num_samples in its front
 * part, free space from tail_start on), as a pair of launches: (1) every perturbed cut, whatever its factor, is resampled into the
 * arena's tail (one workgroup = 256 hops of one cut, the polyphase bank selected per cut), the padding rows of the collated tensor are
 * filled and the descriptor table of launch (2) is put in place -- for mini-batches of up to ~100 cuts the tables travel in the kernel
 * arguments, i.e. there is no host -> device copy in front of the launches at all; (2) the feature kernel of `plan` reads every cut
 * where it now lies (unperturbed cuts are never copied) and writes it into its slot of the dense (batch, rows_per_cut, feature_dim)
 * tensor.  Results are bit-identical to hipfeat_resample per factor + hipfeat_extract_collated.
 *
 * A bank = the resamplers a mini-batch may refer to (h_bank_index[b] = index into the bank, -1 = unperturbed); they must be of the
 * compile-time ratios 9:10 and 11:10 (speed 0.9 / 1.1, width 7: the factors of Kaldi-style three-way speed perturbation) -- anything
 * else: HIPFEAT_ERR_UNSUPPORTED, use hipfeat_resample per factor -- and must outlive the bank.
 *
 * hipfeat_minibatch_plan is host arithmetic only: where each perturbed cut goes (h_out_offsets), how long it is (h_out_num_samples;
 * ceil(new * n / orig) as hipfeat_resampled_length, capped by h_max_samples[b] >= 0 when given: lhotse truncates a perturbed cut to
 * the sample count its manifest states, lhotse/audio/recording.py:1058-1060), its frame count (h_num_frames), and in h_info[4] =
 * {ticket, floats the arena must hold, largest frame count, rows of the output} -- what the caller needs to allocate the arena and the
 * output.  zero_pad_batch != 0 frames every cut on a row of the longest cut's length (edge_rule "batch_zero_pad", _extract_batch's rule).
 * SEVERAL mini-batches per launch pair (a prefetching loader: fewer, larger launches fill 256 CUs better than one 600 s mini-batch can):
 * num_groups > 1 and h_group_sizes[k] = cuts of mini-batch k (consecutive cuts; the sizes add up to `batch`).  Every mini-batch then is
 * its own dense (B_k, T_k, feature_dim) tensor, T_k = its longest cut, the tensors back to back in d_out: h_group_rows[2k] = first row,
 * h_group_rows[2k + 1] = T_k; h_info[3] = rows in total.  num_groups <= 1 (h_group_sizes may be NULL): one mini-batch.
 * hipfeat_minibatch_run enqueues the two launches of a planned mini-batch on `stream`; one mini-batch: rows_per_cut >= h_info[2] (the
 * caller may want more rows than the longest cut has); grouped plans: rows_per_cut = -1, d_out holds h_info[3] rows.  Up to 16 plans may
 * be outstanding per bank; a bank may be shared by threads (calls are serialised inside).
 */
typedef struct hipfeat_speed_bank hipfeat_speed_bank;
HIPFEAT_API hipfeat_status hipfeat_speed_bank_create(const hipfeat_resampler* const* resamplers, int32_t num_resamplers,
                                                     hipfeat_speed_bank** bank);
HIPFEAT_API hipfeat_status hipfeat_speed_bank_destroy(hipfeat_speed_bank* bank);
HIPFEAT_API hipfeat_status hipfeat_minibatch_plan(hipfeat_speed_bank* bank, const hipfeat_plan* plan, int64_t batch, const int64_t* h_offsets,
                                                  const int64_t* h_num_samples, const int32_t* h_bank_index, const int64_t* h_max_samples,
                                                  int64_t tail_start, int32_t zero_pad_batch, int64_t num_groups, const int64_t* h_group_sizes,
                                                  int64_t* h_out_offsets, int64_t* h_out_num_samples, int64_t* h_num_frames,
                                                  int64_t* h_group_rows, int64_t* h_info);
HIPFEAT_API hipfeat_status hipfeat_minibatch_run(hipfeat_speed_bank* bank, int64_t ticket, float* d_arena, int64_t arena_floats, float* d_out,
                                                 int64_t rows_per_cut, float pad_value, void* stream);

/* ---- ABI v6: the tracks of MixedCuts mixed on the device (noise at an SNR, padding) ------------------------------ */
/*
 * CutMix / CutSet.mix / CutSet.pad turn a cut into a MixedCut whose samples come out of MixedCut.load_audio (lhotse/cut/mixed.py:1312-1409):
 * every audible track is loaded, audio_energy = mean(x^2) is taken per track (lhotse/audio/mixer.py:175-176), every SNR becomes a gain
 * against the reference track's energy, and AudioMixer adds gain * audio at the tracks' offsets in track order (mixer.py:104-119, 138-172).
 * Here the tracks of a whole mini-batch lie in ONE device arena (unperturbed tracks as packed, speed-perturbed ones where hipfeat_resample
 * put them) and two stream-ordered launches -- sums of squares per track, then gains + the scaled sum -- write the mixed cuts behind
 * them; no value visits the host in between, so hipfeat_extract* over the returned offsets / lengths can follow on the same stream.
 *   E_t = mean(x_t^2) in float64;  g_t = 1 when the track has no SNR, the cut no reference track, E_ref <= 0 or E_t <= 0, or when it is
 *   the first track and the reference itself; else g_t = (float)sqrt(E_ref * 10^(-snr_t / 10) / E_t);
 *   out[i] = ((0 + g_0 * x_0[i - o_0]) + g_1 * x_1[i - o_1]) + ... over the tracks that cover i, float32, product rounded before the add;
 *   samples no track covers are 0; the cut has max_t(o_t + n_t) samples, cut down to h_max_samples[c] when that is >= 0 and smaller
 *   (mixed.py:1381-1385).  Results are bit-identical from run to run and do not depend on the other cuts of the batch.
 *
 * hipfeat_mixer_create / _destroy: the object that owns the workspace (partial sums, staged tables) on `device`; calls are serialised
 * inside, up to 16 plans may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_mix_plan (host only): the tracks of cut c are [h_track_first[c], h_track_first[c + 1]) in the four track tables
 * (h_track_first[0] = 0; 1 ... 256 tracks per cut): h_src_offset = arena offset of the track's samples, -1 = a padding track (PaddingCut: no
 * source, it only lengthens the cut); h_src_len = its samples; h_dst_offset = its first sample inside the cut
 * (compute_num_samples(track.offset)); h_snr_db = its SNR in dB, NaN = none (h_snr_db may be NULL: none at all).  h_ref_track[c] = the
 * SNR reference track (_get_snr_reference_track, mixed.py:1909-1918) as an index WITHIN the cut, -1 = none (may be NULL).  Every source must
 * end at or before tail_start: the mixed cuts are written from there on, each on a 16-byte boundary, at h_out_offsets[c] with
 * h_out_num_samples[c] samples.  h_info[4] = {ticket, floats the arena must hold, energy work items, mix work items}.
 * A bad table (negative offset, a source that reaches into the tail, a reference index outside the cut or on a padding track, an empty
 * cut, a 17th plan while 16 are planned and not yet run) returns HIPFEAT_ERR_INVALID, more than 256 tracks in a cut HIPFEAT_ERR_UNSUPPORTED,
 * and plans nothing.
 * hipfeat_mix_run enqueues the two launches of a planned mix on `stream` (a ticket runs once); an unknown ticket or an arena smaller
 * than h_info[1] returns HIPFEAT_ERR_INVALID and launches nothing.  A ticket is consumed when its launch has been enqueued: after a
 * HIPFEAT_ERR_HIP from an allocation or the table copy in front of it, it can be run again.
 */
typedef struct hipfeat_mixer hipfeat_mixer;
HIPFEAT_API hipfeat_status hipfeat_mixer_create(int32_t device, hipfeat_mixer** mixer);
HIPFEAT_API hipfeat_status hipfeat_mixer_destroy(hipfeat_mixer* mixer);
HIPFEAT_API hipfeat_status hipfeat_mix_plan(hipfeat_mixer* mixer, int64_t num_cuts, const int64_t* h_track_first, const int64_t* h_src_offset,
                                            const int64_t* h_src_len, const int64_t* h_dst_offset, const double* h_snr_db,
                                            const int32_t* h_ref_track, const int64_t* h_max_samples, int64_t tail_start,
                                            int64_t* h_out_offsets, int64_t* h_out_num_samples, int64_t* h_info);
HIPFEAT_API hipfeat_status hipfeat_mix_run(hipfeat_mixer* mixer, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream);

/* ---- ABI v7: cuts reverberated with a recorded room impulse response on the device ------------------------------ */
/*
 * ReverbWithImpulseResponse.__call__ (lhotse/augmentation/rir.py:78-153) scales the loaded RIR by 2^-15, convolves every output channel's
 * input with it through three float32 FFTs of size next_fast_len(N + L - 1) (convolve1d, lhotse/augmentation/utils.py:49-75), keeps the N
 * samples from argmax(rir) on ("shift output", rir.py:145-146) and, with normalize_output, scales them to the input's power (rir.py:148-151).
 * Here the inputs AND the scaled RIRs of a whole mini-batch lie in ONE device arena and two stream-ordered launches -- a direct-form float32
 * convolution that also writes float64 partial sums of squares, then the gain -- write the reverberated channels behind them; no value
 * visits the host in between, so hipfeat_mix_run / hipfeat_extract* over the returned offsets can follow on the same stream.
 * One (input channel, RIR channel) pair is an item:
 *   hs = rir * 2^-15 (exact; done by the caller);  shift = first index of max(hs) (np.argmax: of the values, not the magnitudes);
 *   y[n] = sum_k hs[k] * x[n + shift - k], 0 <= n < N, over the k with 0 <= n + shift - k < N; float32: runs of 16 consecutive taps
 *   [16 s, 16 s + 16) accumulated with fmaf in ascending order, the 16 runs of the 256 taps [256 c, 256 c + 256) added in ascending order into
 *   a partial sum, the partial sums added in ascending order of c (kernel_reverb.hpp has the order in full);
 *   with the normalise flag: Sx = sum x^2, Sy = sum y^2 in float64; if Sy > 0: y *= (float)sqrt((Sx / N) / (Sy / N)), else y stays.
 *   Results are bit-identical from run to run and do not depend on the other items of the batch.
 *
 * hipfeat_reverb_create / _destroy: the object that owns the workspace (partial sums, staged tables) on `device`; calls are serialised
 * inside, up to 16 plans may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_reverb_plan (host only): per item h_src_offset / h_src_len = arena offset and samples N of the input channel, h_rir_offset /
 * h_rir_len = arena offset and taps L of the SCALED impulse response, h_shift, h_normalize (may be NULL: none).  Every source and every
 * impulse response must end at or before tail_start: the outputs are written from there on, each on a 16-byte boundary, N samples at
 * h_out_offsets[i]; sources are never modified.  h_info[4] = {ticket, floats the arena must hold, convolution work items, partial sums}.
 * A bad table (a negative offset, N < 1 or L < 1, a shift outside [0, L), a source or impulse response that reaches past tail_start, a
 * 17th plan while 16 are planned and not yet run) returns HIPFEAT_ERR_INVALID and plans nothing.
 * hipfeat_reverb_run enqueues the two launches of a planned reverberation on `stream` (a ticket runs once); an unknown ticket or an arena
 * smaller than h_info[1] returns HIPFEAT_ERR_INVALID and launches nothing.  A ticket is consumed when its launch has been enqueued: after
 * a HIPFEAT_ERR_HIP from an allocation or the table copy in front of it, it can be run again.
 */
typedef struct hipfeat_reverb hipfeat_reverb;
HIPFEAT_API hipfeat_status hipfeat_reverb_create(int32_t device, hipfeat_reverb** reverb);
HIPFEAT_API hipfeat_status hipfeat_reverb_destroy(hipfeat_reverb* reverb);
HIPFEAT_API hipfeat_status hipfeat_reverb_plan(hipfeat_reverb* reverb, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                               const int64_t* h_rir_offset, const int64_t* h_rir_len, const int64_t* h_shift,
                                               const int32_t* h_normalize, int64_t tail_start, int64_t* h_out_offsets, int64_t* h_info);
HIPFEAT_API hipfeat_status hipfeat_reverb_run(hipfeat_reverb* reverb, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream);

/* ---- the reverberation by partitioned FFT convolution, opt-in per plan (additive to ABI v8) ----------------------- */
/*
 * The same rule (ReverbWithImpulseResponse.__call__, lhotse/augmentation/rir.py:78-153; its convolve1d, lhotse/augmentation/utils.py:49-75,
 * is three float32 FFTs) with the convolution taken as the reference takes it, through FFTs, but block by block: uniformly partitioned
 * overlap-save (kernel_reverb_fft.hpp, reverb_fft_tables.hpp).
 *   Partition geometry: block B = 1024 samples, transform size 2 B = 2048 (one wave per transform).  An item with N samples, L taps and
 *   shift s has P = ceil(L / 1024) partitions h_p = hs[1024 p, 1024 p + 1024) zero-padded to 2048 (spectra H_p), the input blocks
 *   x[1024 (i - 1), 1024 (i + 1)) with zeros outside [0, N), i = 0 ... nx - 1, nx = min(j1, floor((N - 1) / 1024) + 1) + 1 (spectra X_i), and
 *   the output blocks j = floor(s / 1024) ... j1 = floor((s + N - 1) / 1024).
 *   Precision: the spectra and their accumulation are float32; the spectra of the impulse responses and the inverse transform are
 *   computed in float64 and rounded once (the input blocks are transformed in float32).
 *   Summation orders, float32: Y_j = sum_p H_p X_{j-p} over the p with 0 <= p < P and 0 <= j - p < nx, p ASCENDING, per bin
 *   re = fmaf(-h.im, x.im, fmaf(h.re, x.re, re)), im = fmaf(h.im, x.re, fmaf(h.re, x.im, im)); the inverse transform of Y_j (float64), times 2^-11, rounded; its
 *   upper 1024 samples are the full convolution at [1024 j, 1024 j + 1024), of which the part inside [s, s + N) is stored.  Sx = the sum over i
 *   ascending of the float64 sums of squares of x[1024 i, 1024 i + 1024); Sy = the sum over j ascending of the float64 sums of squares of
 *   what block j stored; the gain and its conditions are those of the direct form.  Results are bit-identical from run to run and do
 *   not depend on the other items of the batch.
 *   Workspace formula: a spectrum is 2048 floats (1024 complex bins, the real bin 1024 beside the real bin 0).  The spectra lie in the
 *   caller's arena behind the outputs: 2048 x (sum of P over the DISTINCT (h_rir_offset, h_rir_len) pairs of the ticket's FFT items + sum
 *   of nx over its FFT items) floats; each distinct impulse response is transformed once, however many items share it.
 * hipfeat_reverb_plan_method = hipfeat_reverb_plan with a route per item.  method: 0 direct (exactly hipfeat_reverb_plan), 1 FFT, 2 auto:
 * an item takes the FFT route when its h_rir_len >= min_fft_taps; one ticket may hold items of both routes.  h_info[8] = {ticket, floats
 * the arena must hold INCLUDING the spectra workspace, direct-form work items, partial sums of both routes, transforms of the spectra
 * launch, output blocks of the accumulate-and-invert launch, work items of the FFT items' gain launch, distinct impulse-response spectra}.
 * A method outside 0 ... 2 or a negative min_fft_taps returns HIPFEAT_ERR_INVALID and plans nothing, as every refusal of
 * hipfeat_reverb_plan.  hipfeat_reverb_run runs the ticket on the routes it was planned with; nothing is allocated per call.
 */
HIPFEAT_REVERB_FFT_API hipfeat_status hipfeat_reverb_plan_method(hipfeat_reverb* reverb, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                      const int64_t* h_rir_offset, const int64_t* h_rir_len, const int64_t* h_shift,
                                                      const int32_t* h_normalize, int64_t tail_start, int32_t method, int64_t min_fft_taps,
                                                      int64_t* h_out_offsets, int64_t* h_info);

/* ---- level changes of cuts on the device (additive to ABI v8) ------------------------------------------------------ */
/*
 * v8 libraries built from this commit on also carry hipfeat_level_*; the version number did not change because nothing that existed
 * changed (a caller that needs them looks the symbols up, or catches the loader's error).
 *
 * Volume.__call__ (lhotse/augmentation/torchaudio.py:395-406; what PerturbVolume / cut.perturb_volume append) multiplies the float32
 * samples by (float)factor.  Clipping.__call__ (lhotse/augmentation/clipping.py:28-61; what the Clipping cut transform /
 * cut.clip_amplitude append) takes p = max |x| over everything it is given, leaves the samples alone when p == 0 or
 * 20 * log10(p) < -96, and otherwise computes [x / p] [* g] clip(., -1, 1) | tanh [/ g] [* p] with float32 array operations.
 * Here the cuts of a whole mini-batch lie in ONE device arena and two stream-ordered launches -- max |x| per item, then the ops --
 * change them where they lie or write them elsewhere; no value visits the host in between.
 * An ITEM is h_src_len[i] samples at h_src_offset[i], written to h_dst_offset[i] (== h_src_offset[i]: in place), with a PROGRAM of
 * 1 ... 4 ops [h_op_first[i], h_op_first[i + 1]) of the three op tables (h_op_first[0] = 0), applied to every sample in order:
 *   h_op_kind 0 = SCALE: y = x * h_op_value (one rounded float32 product); h_op_flags 0.
 *   h_op_kind 1 = CLIP:  h_op_flags = 1 (hard; else soft) | 2 (normalize) | 4 (use the gain: the caller sets it when |gain_db| >= 0.1),
 *     h_op_value = g = (float)10^(gain_db / 20).  p = max |x| of the op's INPUT over the item: the peak of the source pushed through the
 *     SCALE ops in front with the same float32 products, p = fl(fl(peak * |f1|) * |f2|), which equals the maximum of the scaled samples
 *     exactly (rounding is monotone and odd).  p == 0 or p < 0x1.09e69ep-16 (the float32 values for which the reference's dB test says
 *     silence): y = x.  Else, float32, in this order: x / p if normalize; * g if gain; clamp(., -1, 1) when hard, else the float64 tanh
 *     rounded once to float32; / g if gain; * p if normalize.  Divisions are IEEE divisions, never products with a reciprocal.
 *     SCALE and hard CLIP reproduce the reference bit for bit; a NaN sample does not raise the peak (in the reference it turns the
 *     whole output into NaN).  A program holds at most one CLIP.
 *   Results are bit-identical from run to run and do not depend on the other items of the batch.
 *
 * hipfeat_level_create / _destroy: the object that owns the workspace (partial peaks, staged table) on `device`; calls are serialised
 * inside, up to 16 plans may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_level_plan (host only).  h_info[4] = {ticket, floats the arena must hold, peak work items, apply work items}.  A bad table (a
 * negative offset, h_src_len < 1 -- np.max of nothing raises in the reference too --, a program of 0 or more than 4 ops, an unknown
 * kind or flag, a gain that is not positive and finite, a destination that overlaps its own source in part or another item's source
 * or destination, a 17th plan while 16 are planned and not yet run) returns HIPFEAT_ERR_INVALID, a second CLIP in a program
 * HIPFEAT_ERR_UNSUPPORTED, and plans nothing.  num_items == 0 is a valid plan whose run launches nothing.
 * hipfeat_level_run enqueues the launches of a planned level change on `stream` (a ticket runs once; the peak launch is left out when
 * no program has a CLIP); an unknown ticket or an arena smaller than h_info[1] returns HIPFEAT_ERR_INVALID and launches nothing.  A ticket
 * is consumed when its launches have been enqueued: after a HIPFEAT_ERR_HIP from an allocation or the table copy in front of them it can
 * be run again.
 */
typedef struct hipfeat_level hipfeat_level;
HIPFEAT_LEVEL_API hipfeat_status hipfeat_level_create(int32_t device, hipfeat_level** level);
HIPFEAT_LEVEL_API hipfeat_status hipfeat_level_destroy(hipfeat_level* level);
HIPFEAT_LEVEL_API hipfeat_status hipfeat_level_plan(hipfeat_level* level, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                              const int64_t* h_dst_offset, const int64_t* h_op_first, const int32_t* h_op_kind,
                                              const float* h_op_value, const int32_t* h_op_flags, int64_t* h_info);
HIPFEAT_LEVEL_API hipfeat_status hipfeat_level_run(hipfeat_level* level, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream);

/* ---- collation of cuts on the device (additive to ABI v8) ----------------------------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_collate_*; as with hipfeat_level_*, the version number did not change
 * because nothing that existed changed.
 *
 * collate_audio (lhotse/dataset/collation.py:148-260) pads the cuts of a mini-batch to the longest one (cuts.pad) and stacks them with
 * collate_vectors(..., padding_value=0.0); it is what AudioSamples.__call__ (lhotse/dataset/input_strategies.py:208-299) returns and what
 * return_audio=True of the feature input strategies collates on the host.  Here the cuts already lie in ONE device arena (where the
 * augmentation chain left them) and ONE launch writes the dense zero-padded tensor; no value visits the host.
 * Row r of `out` (num_rows x row_len elements, dense) receives the h_src_len[r] float32 samples at arena + h_src_offset[r], starting at
 * element h_dst_offset[r] of the row (NULL = 0 for every row: right padding; row_len - h_src_len[r]: left padding).  Every other element
 * of the row is written as +0.  Every element of out[0 : num_rows * row_len] is written exactly once by the launch (no memset in front of
 * it), nothing outside that range is written and nothing of the arena is written.  out_type 0 = float32: a bit copy; 1 = binary16,
 * 2 = bfloat16: one round-to-nearest-even conversion per sample (the value torch's .to(dtype) gives).  All element indexing is 64-bit.
 *
 * hipfeat_collate_create / _destroy: the object that owns the staged row table on `device`; calls are serialised inside, up to 16 plans
 * may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_collate_plan (host only).  h_info[4] = {ticket, floats the arena must hold (rows of no samples do not count), elements `out`
 * must hold (num_rows * row_len), work items}.  A negative h_src_offset or h_dst_offset, h_src_len < 0, row_len < 0, num_rows < 0,
 * h_dst_offset + h_src_len > row_len, num_rows * row_len or h_src_offset + h_src_len beyond INT64_MAX, an unknown out_type, a 17th plan
 * while 16 are planned and not yet run: HIPFEAT_ERR_INVALID, and nothing is planned.  h_src_len == 0 (a row of padding only) and
 * num_rows == 0 (a plan whose run launches nothing) are valid.
 * hipfeat_collate_run enqueues the launch of a planned collation on `stream` (a ticket runs once).  An unknown ticket, arena_floats <
 * h_info[1], out_elements < h_info[2], or an `out` whose byte range [d_out, d_out + out_elements * size) overlaps the arena's
 * [d_arena, d_arena + 4 * arena_floats): HIPFEAT_ERR_INVALID, and nothing is launched.  The arena starts on a 16-byte boundary, `out` on
 * a multiple of its element size.  A ticket is consumed when its launch has been enqueued: after a HIPFEAT_ERR_HIP from an allocation
 * or the table copy in front of it, it can be run again.
 */
typedef struct hipfeat_collate hipfeat_collate;
HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_create(int32_t device, hipfeat_collate** collate);
HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_destroy(hipfeat_collate* collate);
HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_plan(hipfeat_collate* collate, int64_t num_rows, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                        const int64_t* h_dst_offset, int64_t row_len, int32_t out_type, int64_t* h_info);
HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_run(hipfeat_collate* collate, int64_t ticket, const float* d_arena, int64_t arena_floats, void* d_out,
                                                       int64_t out_elements, void* stream);

/* ---- collation of multi-channel cuts: (B, C, T) and the mono downmix (additive to ABI v8) --------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_collate_plan_sources; as with hipfeat_level_* and hipfeat_collate_*, the
 * version number did not change because nothing that existed changed.
 *
 * collate_audio (lhotse/dataset/collation.py:215-241) either downmixes a multi-channel cut to mono, audio.mean(dim=0) of its (C, T)
 * samples, and collates (B, T), or collates (B, C, T) with all-zero rows for the channels a cut does not have.  Both are ONE launch of a
 * second plan form of hipfeat_collate: output row r has k_r = h_first[r + 1] - h_first[r] >= 0 sources, each a run of h_src_len[r]
 * float32 samples of the arena, source c at arena + h_src_offset[h_first[r] + c]; the row receives, from element h_dst_offset[r]
 * (NULL = 0 for every row), per sample i
 *   k = 0: nothing, the row is +0 everywhere;
 *   k = 1: source 0, exactly the row of hipfeat_collate_plan (float32: a bit copy);
 *   k >= 2: float32((0.0 + double(x_0[i]) + ... + double(x_{k-1}[i])) / double(k)): the sum in ascending source order in float64, one
 *           float64 division, ONE rounding to nearest even (for sources whose float64 sum is exact, such as PCM samples, the correctly
 *           rounded mean, which no float32 summation order is); binary16 / bfloat16 output converts that float32 value as it converts a
 *           sample, so the result is .to(dtype) of the float32 mean.  NaN and Inf propagate by the IEEE rules.
 * Every other element of the row is +0; what is written and what is not is as for hipfeat_collate_plan.  (B, T): one row per cut with
 * its channels as sources.  (B, C, T): B * C rows of one source, or none.
 *
 * hipfeat_collate_plan_sources (host only).  h_first[num_rows + 1], h_src_offset[h_first[num_rows]], h_src_len[num_rows]; h_info[4] as
 * hipfeat_collate_plan: {ticket, floats the arena must hold (the sources of rows with h_src_len == 0 do not count), elements `out` must
 * hold (num_rows * row_len), work items}.  h_first that does not start at 0 or decreases, a negative offset or length, row_len < 0,
 * num_rows < 0, h_dst_offset + h_src_len > row_len, num_rows * row_len or h_src_offset + h_src_len beyond INT64_MAX, an unknown
 * out_type, a 17th plan while 16 are planned and not yet run: HIPFEAT_ERR_INVALID; a row of more than 32 sources:
 * HIPFEAT_ERR_UNSUPPORTED; nothing is planned.  The tickets are those of hipfeat_collate_plan: hipfeat_collate_run runs a ticket of
 * either form, with the same checks.
 */
HIPFEAT_CHANNELS_API hipfeat_status hipfeat_collate_plan_sources(hipfeat_collate* collate, int64_t num_rows, const int64_t* h_first,
                                                                 const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset,
                                                                 int64_t row_len, int32_t out_type, int64_t* h_info);

/* ---- sinc resampling without a filter bank: any rate pair, every row with its own (additive to ABI v8) ------------------------ */
/*
 * v8 libraries built from this commit on also carry hipfeat_sinc_*.  What they replace: ResampleTensor = _get_sinc_resample_kernel +
 * _apply_sinc_resample_kernel (lhotse/augmentation/resample.py:184-315) for rate pairs whose dense filter bank (new x (2 width + orig)
 * weights, rates reduced by their gcd) is too large to build -- the two Resample transforms that LowpassUsingResampling appends
 * (lhotse/dataset/cut_transforms/lowpass.py: Resample(sr -> 2c), Resample(2c -> sr), a random integer cutoff c per cut; 16000 -> 9346 is
 * 8000 : 4673, a bank of 37.5 M weights of which 22 per phase are not zero), and any Resample (lhotse/augmentation/torchaudio.py:86-139)
 * between such rates.  The weights of the reference (resample.py:239-281; hann window, lowpass_filter_width 6, rolloff 0.99) are
 * evaluated on the device where they are not zero, in float64 rounded once to float32, per launch; nothing grows with the rates.
 * Row r of a launch takes the h_in_len[r] samples at arena + h_in_offset[r] from h_src_rate[r] to h_dst_rate[r] (unreduced) and writes
 * h_out_len[r] = hipfeat_resampled_length(h_in_len[r], src, dst) samples (resample.py:309) at arena + h_out_offset[r]; each output is
 * the ascending-tap fmaf chain of hipfeat_resample over the taps whose weight is not zero.  All offsets are 64-bit.
 *
 * hipfeat_sinc_create / _destroy: the object that owns the staged row table on `device`; calls are serialised inside, up to 16 plans
 * may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_sinc_plan (host only) writes h_out_len[num_rows] and h_info[4] = {ticket, floats the arena must hold, workgroups, largest
 * window W = 2 width + 2 of the rows}.  Refused, and nothing planned: a rate <= 0, equal rates, a negative offset or length, an input
 * or output range past arena_floats, an output range that overlaps any row's input range (its own included) or another row's output, a
 * 17th plan while 16 are planned and not yet run: HIPFEAT_ERR_INVALID; a rate pair whose window exceeds 96 taps (width > 47: a
 * downsampling ratio beyond 7.75) or whose reduced rates exceed 2^24: HIPFEAT_ERR_UNSUPPORTED.  Rows of no samples and num_rows == 0 are valid.
 * hipfeat_sinc_run enqueues the ONE launch of a planned resampling on `stream` (a ticket runs once).  An unknown ticket or arena_floats
 * < h_info[1]: HIPFEAT_ERR_INVALID, nothing is launched.  The arena starts on a 16-byte boundary.
 * hipfeat_sinc_weights: the filter a rate pair gets here, for inspection: h_dims[3] = {new, W, width} (host, written at once),
 * d_weights[new][W] float32 and d_first[new] int32, the window's first tap counted in taps of the zero-padded input (resample.py:307);
 * tap d of phase ph is the reference's kernel[ph][d_first[ph] + d].  d_weights == d_first == NULL: the sizes alone.
 */
typedef struct hipfeat_sinc hipfeat_sinc;
HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_create(int32_t device, hipfeat_sinc** sinc);
HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_destroy(hipfeat_sinc* sinc);
HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_plan(hipfeat_sinc* sinc, int64_t num_rows, const int64_t* h_in_offset, const int64_t* h_in_len,
                                                  const int32_t* h_src_rate, const int32_t* h_dst_rate, const int64_t* h_out_offset,
                                                  int64_t arena_floats, int64_t* h_out_len, int64_t* h_info);
HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_run(hipfeat_sinc* sinc, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream);
HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_weights(hipfeat_sinc* sinc, int32_t src_rate, int32_t dst_rate, float* d_weights, int32_t* d_first,
                                                     int32_t* h_dims, void* stream);

/* ---- stored features mixed and collated on the device (additive to ABI v8) -------------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_featmix_*; as with hipfeat_level_* and hipfeat_collate_*, the version number
 * did not change because nothing that existed changed.
 *
 * PrecomputedFeatures.__call__ -> collate_features (lhotse/dataset/collation.py:115-145) pads every cut of a mini-batch (cuts.pad) and
 * fills row c of a (B, max num_frames, F) float32 tensor with cut.load_features(), cut by cut on the host.  For a MixedCut that call
 * (lhotse/cut/mixed.py:1199-1309) loads every track and runs FeatureMixer (lhotse/features/mixer.py) with Fbank.mix / Fbank.compute_energy
 * (lhotse/features/kaldi/extractors.py:135-152).  Here the tracks of the whole mini-batch lie in ONE device arena AS THEY WERE STORED
 * (float32 or binary16) and two stream-ordered launches -- sum(exp(x)) per track that needs one, then the fold and the padded batch --
 * write the (num_cuts, row_frames, F) tensor; no value visits the host in between, no memset, no intermediate matrix.
 * EPSILON = 1e-10 (lhotse.utils).  A cut has one of two forms:
 *   COPY (form 0; mixed.py:1223-1243: a plain cut, or one cut with PaddingCuts behind it): ONE track; the cut's first h_frames frames are
 *     bit copies of the track (binary16 widened exactly; a constant track: (float)h_value), its other frames (float)h_pad_value.
 *   FOLD (form 1; mixed.py:1245-1307): tracks t = 0 ... K-1 in order; track t is a matrix x_t of n_t = h_frames frames (or a constant
 *     matrix, a PaddingCut) that starts at frame o_t = h_first (compute_num_frames(track.offset, frame_shift, sampling_rate)).
 *     N = max_t(o_t + n_t); a frame a track does not cover holds the mixer's padding value -1000, whose exp is 0.
 *     S(x) = sum(exp(x)) over a track's own frames, in float64.  E_ref = S(x_ref), ref = h_ref_track (_get_snr_reference_track,
 *     mixed.py:1909-1918).  Gains: a track with an SNR (track 0 only when the reference is another track; _scale_features_for_snr,
 *     mixed.py:1945-1957; mixer.py:168-175) gets g_t = (float)(E_ref * 10^(-snr_t/10) / S(x_t)) when E_ref > 0 and S(x_t) > 0, every
 *     other track and every other case g_t = 1.
 *     Per frame and bin, float32: e = g_0 * exp(x_0); for t = 1 ... K-1 in order: e = max(EPSILON, e + g_t * exp(x_t)) -- the floor
 *     after EVERY track over ALL N frames (a frame only a later track covers already holds 1e-10 when that track arrives; a tail two
 *     paddings cover ends at log(2e-10)); a track t >= 1 of no frames is not mixed at all (mixer.py:116-117).  out = log(e), taken once.
 *     N - h_num_frames == +1: the last frame is dropped; == -1: the last frame is repeated (mixed.py:1294-1300).
 *   The MonoCut fix-up (lhotse/cut/mono.py:61-64) is per track: h_src_rows stored rows stand for h_frames frames; one row too many is
 *   not read, one too few repeats the last row (energies are those of the fixed-up matrix).
 *   The cut's h_num_frames frames go to frames [h_dst_first, h_dst_first + h_num_frames) of row c; every other element of the row is
 *   (float)log(1e-10).  Results are bit-identical from run to run and a cut's row does not depend on the other cuts of the batch.
 *
 * hipfeat_featmix_create / _destroy: the object that owns the workspace (staged tables, partial sums) on `device`; calls are serialised
 * inside, up to 16 plans may be outstanding, destroy waits for the work it enqueued.
 * hipfeat_featmix_plan (host only): the tracks of cut c are [h_track_first[c], h_track_first[c + 1]) of the track tables
 * (h_track_first[0] = 0; 1 ... 256 tracks per cut, exactly 1 in the copy form).  Per cut: h_form, h_num_frames, h_pad_value (may be NULL:
 * 0), h_dst_first (may be NULL: 0), h_ref_track = the SNR reference as an index WITHIN the cut, -1 = none (may be NULL).  Per track:
 * h_src_offset = BYTE offset of its first stored value in the arena (a multiple of 4 for float32, of 2 for binary16), -1 = a constant
 * track; h_src_rows (may be NULL: h_frames); h_frames; h_dtype 0 = float32, 1 = binary16 (may be NULL: float32); h_first (may be NULL: 0);
 * h_snr_db, NaN = none (may be NULL); h_value of constant tracks (may be NULL: 0).  num_features = F >= 1 (any value); row_frames = the
 * frames of one row of `out`.  h_info[4] = {ticket, bytes the arena must hold, energy work items, fold work items}.
 * A bad table (a negative or misaligned offset, frames that do not fit the row, h_src_rows further than one from h_frames, a mix whose
 * length is further than one from h_num_frames, a reference index outside the cut, an unknown form or type, a copy form with more than one
 * track, a 17th plan while 16 are planned and not yet run) returns HIPFEAT_ERR_INVALID, more than 256 tracks in a cut
 * HIPFEAT_ERR_UNSUPPORTED, and plans nothing.
 * hipfeat_featmix_run enqueues the two launches of a planned feature mix on `stream` (a ticket runs once; the energy launch is left out
 * when no track needs an energy).  An unknown ticket, arena_bytes < h_info[1], out_elements < num_cuts * row_frames * F, or an `out`
 * that overlaps the arena: HIPFEAT_ERR_INVALID, and nothing is launched.  The arena starts on a 16-byte boundary, `out` on a 4-byte one.
 * A ticket is consumed when its launches have been enqueued: after a HIPFEAT_ERR_HIP from an allocation or the table copy in front of
 * them, it can be run again.
 */
typedef struct hipfeat_featmix hipfeat_featmix;
HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_create(int32_t device, hipfeat_featmix** featmix);
HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_destroy(hipfeat_featmix* featmix);
HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_plan(hipfeat_featmix* featmix, int64_t num_cuts, const int64_t* h_track_first, const int32_t* h_form,
                                                        const int64_t* h_num_frames, const double* h_pad_value, const int64_t* h_dst_first,
                                                        const int32_t* h_ref_track, const int64_t* h_src_offset, const int64_t* h_src_rows,
                                                        const int64_t* h_frames, const int32_t* h_dtype, const int64_t* h_first, const double* h_snr_db,
                                                        const double* h_value, int64_t num_features, int64_t row_frames, int64_t* h_info);
HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_run(hipfeat_featmix* featmix, int64_t ticket, const void* d_arena, int64_t arena_bytes, float* d_out,
                                                       int64_t out_elements, void* stream);

/* ---- global feature statistics on the device (additive to ABI v8) ----------------------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_stats_*; the version number did not change because nothing that existed
 * changed.
 *
 * CutSet.compute_global_feature_stats (lhotse/cut/set.py:2533-2583) hands one feature matrix per cut to StatsAccumulator.update
 * (lhotse/features/base.py:957-1033), float64 numpy on the host.  Here the matrices of many cuts lie in ONE device buffer, float32
 * (dtype 0) or IEEE binary16 (dtype 1), row-major with row_stride >= feature_dim ELEMENTS per row; cut b owns the rows
 * [h_first_row[b], h_first_row[b] + h_num_frames[b]) -- the packed (sum T, F) matrix hipfeat_extract writes as well as a padded
 * (B, Tmax, F) tensor, whose padding rows are never read.  Rows need not ascend; h_first_row * row_stride may exceed 2^31.
 *
 * State: total_frames (int64, also known to the host), total_sum[F], total_unnorm_var[F] (float64, on the device).  Cut by cut, in the
 * order of the table, all in float64:
 *   curr_sum = sum(x), curr_unnorm_var = sum((x - mean_cut)^2) (= np.var(x, axis=0) * curr_frames; E[x^2] - E[x]^2 is never formed);
 *   total_frames > 0:  r = total_frames / curr_frames;
 *                      total_unnorm_var = total_unnorm_var + curr_unnorm_var + r / (total_frames + curr_frames) * (total_sum / r - curr_sum)^2
 *   total_frames == 0: total_unnorm_var = curr_unnorm_var                      (the first cut into an empty state assigns)
 *   total_sum = total_sum + curr_sum;  total_frames = total_frames + curr_frames.
 * A cut is summed in blocks of 256 frames (block sums about the block's own mean), and its blocks are merged in block order with
 * the pairwise update of Chan, Golub and LeVeque; no floating-point atomic is used, the order is the table's, so the result is bit-identical
 * from run to run and does not depend on how the cuts were grouped into updates.  A cut of 0 frames contributes NOTHING (the reference's
 * np.var of an empty matrix would turn every bin into NaN).  Non-finite values propagate as float64 arithmetic makes them, in their
 * own bin only.
 *
 * hipfeat_stats_create / _destroy: the object that owns the state, the slab of block partials (grows on demand) and 16 staging slots on
 * `device`, for feature_dim = 1 ... 65535 bins; calls are serialised inside; destroy waits for the work it enqueued; destroying NULL is OK.
 * hipfeat_stats_update validates on the host, stages the table and enqueues the two launches on `stream` without waiting (a 17th update
 * waits for the first one's launches; an update that needs a larger slab than every one before it -- never the first -- waits for the
 * launches of all earlier updates before the old slab is freed).  1 ... 65535 cuts; h_first_row == NULL: the cuts are packed back to back from row 0.  Negative
 * rows or frames, row_stride < feature_dim, a cut whose last element lies beyond feats_elems, a dtype other than 0 or 1, a base pointer
 * that is not a multiple of the element size (the stride counts elements and cannot break it), counts out of range:
 * HIPFEAT_ERR_INVALID; more than 2^24 blocks in one update: HIPFEAT_ERR_UNSUPPORTED; nothing is enqueued and the state is unchanged.
 * The calls of one object are meant for ONE stream at a time: the host's total_frames is that of what has been enqueued.
 * hipfeat_stats_merge folds another accumulator's state (host arrays of feature_dim float64 each) in with the update above, `frames`
 * standing for curr_frames: the ranks of a sharded pass combine their parts.  frames == 0 is a no-op.
 * hipfeat_stats_get waits for `stream` and copies the state out (any of the three pointers may be NULL).
 * hipfeat_stats_reset zeroes the state.  Every call on a NULL object is HIPFEAT_ERR_INVALID and needs no device.
 */
typedef struct hipfeat_stats hipfeat_stats;
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_create(int32_t device, int32_t feature_dim, hipfeat_stats** stats);
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_destroy(hipfeat_stats* stats);
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_update(hipfeat_stats* stats, const void* d_feats, int64_t feats_elems, int32_t dtype,
                                                      int64_t num_cuts, const int64_t* h_first_row, const int64_t* h_num_frames,
                                                      int64_t row_stride, void* stream);
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_merge(hipfeat_stats* stats, int64_t frames, const double* h_sum, const double* h_unnorm_var, void* stream);
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_get(hipfeat_stats* stats, int64_t* h_frames, double* h_sum, double* h_unnorm_var, void* stream);
HIPFEAT_STATS_API hipfeat_status hipfeat_stats_reset(hipfeat_stats* stats, void* stream);

/* ---- Kaldi frames and their complex STFT on the device (additive to ABI v8) --------------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_stft_*; the version number did not change because nothing that existed
 * changed.
 *
 * The two layers of lhotse/features/kaldi/layers.py whose output is not a real feature matrix: Wav2Win (layers.py:151-197), the
 * preprocessed frames, and Wav2FFT (layers.py:309-324), their complex spectrum.  One launch maps a (batch, num_samples) float32
 * batch of equally long rows -- row b at d_wave + b * row_stride ELEMENTS, the base 4-byte aligned -- to one of two outputs.
 *
 * HIPFEAT_STFT_FRAMES.  For frame t, tap i < frame_length, in this order:
 *   1. the sample at frame_indices (layers.py:727-772): j = t * frame_shift + i when snip_edges, else j = t * frame_shift + i -
 *      (frame_length - frame_shift) / 2 with the flip-reflection at both ends: j < 0 -> -j - 1, j >= S -> 2 S - 1 - j;
 *   2. minus the mean of the frame if remove_dc_offset (layers.py:155-157); the mean is a float64 sum rounded to float32 once;
 *   3. the raw log-energy max(log(sum x^2 + 1e-15), log(energy_floor)) (layers.py:859-870) if want_energy and raw_energy;
 *   4. pre-emphasis x[i] - c x[max(i - 1, 0)] if preemph_coeff != 0 (layers.py:165-167);
 *   5. times window[i] (layers.py:170);
 *   6. zeros for the taps frame_length ... pad_length - 1 (layers.py:173-181);
 *   7. the log-energy of the windowed frame if want_energy and not raw_energy (layers.py:183-185).
 * d_out is (batch, T, pad_length) float32 with any pad_length >= frame_length, d_log_energy (batch, T) float32 (may be NULL; it is
 * written only when want_energy).  frame_length <= 2048.  Only [d_out, d_out + batch * T * pad_length) is written.
 *
 * HIPFEAT_STFT_SPECTRUM.  The same frame with pad_length = fft_length, then its real FFT (layers.py:314): bins 0 ... fft_length / 2 as
 * interleaved (re, im) float32 pairs, rows of fft_length + 2 floats, d_out 8-byte aligned -- a (batch, T, fft_length / 2 + 1) complex64
 * tensor.  With want_energy bin 0 of every frame is (log_energy, 0) (layers.py:317-318).  fft_length is 256, 512, 1024 or 2048 (8 to 48
 * kHz at 25 ms): a complex FFT of fft_length / 2 points in three register passes plus the split step, in float32; there is no direct-DFT
 * path, whose rounding error is not that of the reference's FFT, so every other pad_length -- the frame_length of
 * round_to_power_of_two=False included -- is HIPFEAT_ERR_UNSUPPORTED at creation.
 *
 * dither must be added by the caller (layers.py:191-193 draws torch.randn).  T = hipfeat_num_frames(num_samples, ...); a row too short
 * for the reflection (hipfeat_check_length) is HIPFEAT_ERR_TOO_SHORT.
 *
 * hipfeat_stft_create validates BEFORE any device call: a NULL argument, a struct_size other than sizeof(hipfeat_stft_config),
 * frame_length <= 0, frame_shift <= 0, pad_length < frame_length, an output other than the two above: HIPFEAT_ERR_INVALID; an unsupported
 * size: HIPFEAT_ERR_UNSUPPORTED.  h_window[frame_length] is copied.  hipfeat_stft_run enqueues one launch on `stream` and waits for
 * nothing; out_floats is the capacity of d_out in floats: smaller than batch * T * row floats is HIPFEAT_ERR_INVALID and nothing is
 * launched, as are negative sizes, row_stride < num_samples with batch > 1, and a NULL or misaligned pointer.  batch == 0, or T == 0 with
 * snip_edges, is HIPFEAT_OK and launches nothing (without snip_edges a row of no frames is too short, as for hipfeat_extract).  Every call on a NULL object is HIPFEAT_ERR_INVALID and needs no device; destroying NULL is OK.
 */
#define HIPFEAT_STFT_FRAMES 0
#define HIPFEAT_STFT_SPECTRUM 1
typedef struct hipfeat_stft_config {
  int32_t struct_size;      /* = sizeof(hipfeat_stft_config); ABI guard                  */
  int32_t output;           /* HIPFEAT_STFT_FRAMES or HIPFEAT_STFT_SPECTRUM              */
  int32_t frame_length;     /* N = floor(frame_length_s * sampling_rate) layers.py:114   */
  int32_t frame_shift;      /* floor(frame_shift_s * sampling_rate)      layers.py:116   */
  int32_t pad_length;       /* layers.py:121; the fft_length of Wav2FFT  layers.py:265   */
  int32_t snip_edges;       /* layers.py:747-753                                         */
  int32_t remove_dc_offset; /* layers.py:155-157                                         */
  int32_t raw_energy;       /* layers.py:161 vs :183                                     */
  int32_t want_energy;      /* return_log_energy / use_energy            layers.py:107   */
  float preemph_coeff;      /* 0 disables                                layers.py:165   */
  float energy_floor;       /* floored at log(energy_floor) if > 0       layers.py:864   */
} hipfeat_stft_config;
typedef struct hipfeat_stft hipfeat_stft;
HIPFEAT_STFT_API hipfeat_status hipfeat_stft_create(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_stft** out);
HIPFEAT_STFT_API hipfeat_status hipfeat_stft_destroy(hipfeat_stft* stft);
HIPFEAT_STFT_API hipfeat_status hipfeat_stft_run(hipfeat_stft* stft, const float* d_wave, int64_t batch, int64_t num_samples, int64_t row_stride,
                                                 float* d_out, int64_t out_floats, float* d_log_energy, void* stream);
/*
 * hipfeat_stft_run_ragged (additive to ABI v8, HIPFEAT_RAGGED_API): the same launch for a zero-padded (batch, max_samples) batch whose row b
 * holds h_lengths[b] <= max_samples samples.  It replaces the reference layer applied to x[b, :len_b] row by row (layers.py:59-333) plus
 * collate_matrices: row b is framed as x[b, :len_b] alone -- T_b = hipfeat_num_frames(len_b, ...) frames, the flip-reflection at both of
 * ITS ends, no sample from len_b on is read -- into a (batch, Tmax, row) output, Tmax = max_b T_b, whose rows T_b ... Tmax - 1 hold
 * padding_value (the spectrum: (padding_value, 0) per bin), as do the log-energies there.  The one launch writes every element; there is no
 * memset and no fill launch.  h_lengths is a HOST array of `batch` int64: it is checked here (negative or > max_samples:
 * HIPFEAT_ERR_INVALID; without snip_edges a row too short for its reflection, a row of no samples included: HIPFEAT_ERR_TOO_SHORT; both
 * name the row) and then staged to the device through a slot of the handle (the kernel reads only lengths this call has checked).  With
 * snip_edges a row shorter than a frame has no frames and is legal; Tmax == 0 launches nothing.  Everything else as hipfeat_stft_run,
 * with max_samples in the place of num_samples; every refusal comes before any device call.
 */
HIPFEAT_RAGGED_API hipfeat_status hipfeat_stft_run_ragged(hipfeat_stft* stft, const float* d_wave, int64_t batch, int64_t max_samples, int64_t row_stride,
                                                          const int64_t* h_lengths, float padding_value, float* d_out, int64_t out_floats,
                                                          float* d_log_energy, void* stream);

/* ---- streaming layers: online_inference of the six Kaldi layers (additive to ABI v8) ------------------------------------- */
/*
 * v8 libraries built from this commit on also carry hipfeat_stream_*; the version number did not change because nothing that existed
 * changed.
 *
 * Every layer of lhotse/features/kaldi/layers.py has online_inference(x, context=None) next to forward (layers.py:199-224, 326-333 and
 * 775-856): a chunk x of chunk_len = S samples per row is framed together with what the previous call left over, and what this call
 * leaves over is returned.  One launch does all of it.  With N = frame_length, s = frame_shift, P = (N - s) / 2:
 *
 *   virtual waveform  V = [A | x] of L = R + S samples.  A is the context, R = context_len samples per row (ANY R >= 0, not only a
 *                     remainder this library returned), when d_context is not NULL.  d_context == NULL is the start of a stream:
 *                     A is empty with snip_edges, else the flipped head of the chunk, R = min(P, S), A(j) = x[R - 1 - j] -- a first chunk
 *                     shorter than P reflects only what it has.  Index map: V(j) = A(j) for j < R, x[j - R] otherwise.
 *   frames            frame f is V[f s : f s + N] for f < T, T = 1 + (L - N) / s when L >= N -- the same number under both snip_edges
 *                     values.  A stream has no end, so nothing is ever reflected on the right.
 *   per frame         the arithmetic of hipfeat_stft_run (frames, spectrum) or of the wave-per-frame feature kernel (the four kinds of
 *                     hipfeat_config), by one wave from the frame's own samples alone: the output of a stream does not depend on how it
 *                     was cut into chunks, bit for bit.
 *   remainder         V[T s : L], L - T s < N samples per row, written to row b of d_remainder, a contiguous (batch, L - T s) matrix.
 *   zero-frame rule   L < N: T = 0, nothing is written to d_out, and all of V is the remainder.  (The reference raises there; this lets a
 *                     caller feed chunks shorter than a frame.)
 *
 * hipfeat_stream_counts is host arithmetic and needs no device: T and the remainder length of one call; `first` != 0 is the start of a
 * stream (context_len must be 0 then).  hipfeat_stream_create_stft takes the configuration of hipfeat_stft_create (frames of any
 * pad_length, or the spectrum), hipfeat_stream_create_features that of hipfeat_plan_create for the kinds HIPFEAT_SPECTROGRAM ...
 * HIPFEAT_MFCC; the feature handle builds the wave-per-frame kernel's tables itself and serves EVERY supported configuration with that
 * one kernel body (one arithmetic for every chunking), also where hipfeat_extract picks a specialised kernel -- so a streamed feature
 * row agrees with hipfeat_extract's to rounding, not bit for bit.  Rows: context row b at d_context + b * context_stride ELEMENTS, chunk
 * row b at d_chunk + b * chunk_stride, any stride >= the row, bases 4-byte aligned; d_out as for hipfeat_stft_run (the spectrum 8-byte
 * aligned) or (batch, T, feature_dim) float32; d_log_energy (batch, T) is written by a frames handle with want_energy (may be NULL) and
 * by no other.  dither must be added to the chunk by the caller.
 *
 * Statuses, as for hipfeat_stft_*: NULL arguments, negative sizes, a NULL context with context_len != 0, misaligned pointers, buffers
 * smaller than batch * T * row / batch * (L - T s) floats and (batch > 1) a stride shorter than its row are HIPFEAT_ERR_INVALID and
 * launch nothing; an fft_length other than 256, 512, 1024 or 2048, frames of more than 2048 samples, more than 128 filters, frame_shift >
 * frame_length, kinds beyond the four and a device that is not a gfx950 are HIPFEAT_ERR_UNSUPPORTED.  Every refusal that does not depend
 * on the device comes BEFORE any device call.  batch == 0 is HIPFEAT_OK and launches nothing.  Every call on a NULL object is
 * HIPFEAT_ERR_INVALID and needs no device; destroying NULL is OK.
 */
typedef struct hipfeat_stream hipfeat_stream;
HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_counts(int32_t frame_length, int32_t frame_shift, int32_t snip_edges, int32_t first,
                                                        int64_t context_len, int64_t chunk_len, int64_t* frames, int64_t* remainder_len);
HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_create_features(const hipfeat_config* cfg, const float* h_window, const float* h_mel,
                                                                 const float* h_dct, const float* h_lifter, int32_t device, hipfeat_stream** out);
HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_create_stft(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_stream** out);
HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_run(hipfeat_stream* stream_handle, const float* d_context, int64_t context_len, int64_t context_stride,
                                                     const float* d_chunk, int64_t chunk_len, int64_t chunk_stride, int64_t batch, float* d_out,
                                                     int64_t out_floats, float* d_log_energy, float* d_remainder, int64_t remainder_floats, void* stream);
HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_destroy(hipfeat_stream* stream_handle);

/* ---- waveform gradient of the six Kaldi layers (additive to ABI v8) ------------------------------------------------------ */
/*
 * v8 libraries built from this commit on also carry hipfeat_grad_*; the version number did not change because nothing that existed
 * changed.  No new config struct: a gradient handle takes the hipfeat_config of hipfeat_stream_create_features (the four kinds
 * HIPFEAT_SPECTROGRAM ... HIPFEAT_MFCC) or the hipfeat_stft_config of hipfeat_stream_create_stft (frames, spectrum), under the limits of
 * the streaming kernels: fft_length 256, 512, 1024 or 2048, frames of at most 2048 samples, at most 128 filters, frame_shift <=
 * frame_length.
 *
 * Every parameter of the reference layers has requires_grad=False; the only gradient there is is the one with respect to the waveform,
 * and its definition is the autograd of lhotse/features/kaldi/layers.py.  Per frame t with gathered samples s_i, i < N, the forward is
 * that of hipfeat_stft_run: d = s - mean(s) (layers.py:155-157), e_raw = max(log(sum d^2 + 1e-15), log floor) (layers.py:859-870),
 * p_i = d_i - c d_{max(i-1,0)} (layers.py:165-167), w_i = p_i win_i with zeros up to pad / fft (layers.py:170-181), e_win the same energy
 * on w (layers.py:183-185), X = rfft(w) (layers.py:314).  The backward, in this order:
 *
 *   1. seed        Gbar_k, k = 0 ... fft / 2, from the output cotangent ybar.  Power: Gbar = 2 Pbar X; magnitude: Gbar = Mbar X / |X|, 0
 *                  where X = 0 (layers.py:38-42).  Log: Pbar = ybar / (P + 1e-15) (layers.py:466-468).  Mel: Pbar_k = sum_m fb[k,m] ybar_m
 *                  [mel_m > eps] / mel_m with mel_m recomputed and eps = mel_floor (layers.py:571-572).  MFCC: first ybar_mel = dct (lifter *
 *                  cbar) (layers.py:708-722).  Where use_energy puts the log-energy into bin 0 / column 0 (layers.py:317, 399, 470; the
 *                  prepended column of layers.py:575; C0 of HIPFEAT_MFCC) that element's cotangent is ebar and seeds no bin.  The spectrum's
 *                  cotangent is complex in torch's convention: for a real loss with dL = sum a dRe X + b dIm X it is a + ib, interleaved
 *                  (re, im) pairs, no factor 2 and no 1 / fft.
 *   2. adjoint FFT wbar_n = sum_k Re(Gbar_k e^{+2 pi i k n / fft}) for n < N: the imaginary parts of bins 0 and fft / 2 drop out, the adjoint
 *                  of zero padding is truncation.  Computed as the adjoint split step and the forward's three register passes on
 *                  conjugated data; there is no direct DFT.  A frames handle starts here with wbar = its cotangent.
 *   3. front end   wbar_i += 2 w_i ebar / (sum w^2 + 1e-15) when the windowed energy was used and not floored; pbar = win wbar;
 *                  dbar_i = pbar_i - c pbar_{i+1} for i < N - 1, dbar_{N-1} = pbar_{N-1}, and dbar_0 additionally gets -c pbar_0 (the replicate
 *                  pad of layers.py:166); dbar_i += 2 d_i ebar / (sum d^2 + 1e-15) for the raw energy when not floored; sbar = dbar -
 *                  mean(dbar) with remove_dc_offset.
 *   4. overlap-add sample j of a row receives sbar_{t,i} from every (t, i) whose index lands on j; the index map is that of
 *                  layers.py:747-772 (snip_edges, or the flip-reflection at both ends: j' = t shift - npad_left + i, j' < 0 -> -j' - 1,
 *                  j' >= S -> 2 S - 1 - j').  The sum runs in a fixed order: ascending t, the direct contribution before the reflected one.
 *                  Samples no frame reads get exactly 0.0.  Every element of d_grad_wave[b][0 .. num_samples) is written.
 *
 * Two launches per piece of rows on `stream`: steps 1-3 write every frame's sbar as a row of Nr = (N + 3) & ~3 floats into the caller's
 * workspace (rows, T, Nr), step 4 gathers it.  No atomics: the gradient of a row is the same bits alone or in any batch, from run to run
 * and under any piece size.  hipfeat_grad_workspace is host arithmetic and touches no device: rows_per_piece = max(1, budget_bytes / (T Nr
 * 4)), at most batch, and floats = rows_per_piece T Nr -- a single row larger than the budget gets a workspace of its own size.
 * hipfeat_grad_run processes workspace_floats / (T Nr) rows per piece, so any workspace that holds one row will do; it must be 16-byte
 * aligned.  d_grad_out is the (batch, T, row) cotangent of the handle's output, contiguous, rows as hipfeat_stream_run writes them
 * (the spectrum: fft_length + 2 floats); for a frames handle it may be NULL (a zero cotangent), as may d_grad_log_energy, the (batch, T)
 * cotangent of its log-energies, which no other handle reads.  Waveform row b at d_wave + b * row_stride ELEMENTS, its gradient at
 * d_grad_wave + b * grad_wave_stride.  dither: the caller adds it and passes the dithered waveform.
 *
 * Statuses, as for hipfeat_stft_* / hipfeat_stream_*: NULL arguments, negative sizes, misaligned pointers, a cotangent smaller than batch
 * * T * row floats, a workspace smaller than one row's T Nr floats and (batch > 1) a stride shorter than its row are HIPFEAT_ERR_INVALID
 * and launch nothing; a row too short for the reflection is HIPFEAT_ERR_TOO_SHORT; an unsupported size or kind and a device that is not a
 * gfx950 are HIPFEAT_ERR_UNSUPPORTED.  Every refusal that does not depend on the device comes BEFORE any device call.  batch == 0 is
 * HIPFEAT_OK and launches nothing.  Every call on a NULL object is HIPFEAT_ERR_INVALID and needs no device; destroying NULL is OK.
 */
typedef struct hipfeat_grad hipfeat_grad;
HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_create_features(const hipfeat_config* cfg, const float* h_window, const float* h_mel, const float* h_dct,
                                                             const float* h_lifter, int32_t device, hipfeat_grad** out);
HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_create_stft(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_grad** out);
HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_workspace(const hipfeat_grad* grad, int64_t batch, int64_t num_samples, int64_t budget_bytes,
                                                       int64_t* rows_per_piece, int64_t* floats);
HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_run(hipfeat_grad* grad, const float* d_wave, int64_t batch, int64_t num_samples, int64_t row_stride,
                                                 const float* d_grad_out, int64_t grad_out_floats, const float* d_grad_log_energy, float* d_grad_wave,
                                                 int64_t grad_wave_stride, float* d_workspace, int64_t workspace_floats, void* stream);
HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_destroy(hipfeat_grad* grad);
/*
 * hipfeat_grad_workspace_ragged / hipfeat_grad_run_ragged (additive to ABI v8, HIPFEAT_RAGGED_API): the gradient of
 * hipfeat_stft_run_ragged's batch (and of the four feature kinds on the same rows).  They replace the autograd of the reference layer
 * applied to x[b, :len_b] row by row (layers.py:59-333) plus collate_matrices.  d_grad_out is the (batch, Tmax, row) cotangent and
 * d_grad_log_energy the (batch, Tmax) one, Tmax = max_b T_b; their rows from T_b on are NEVER read.  Row b of d_grad_wave gets the gradient
 * of x[b, :len_b] alone in its first len_b samples -- gathered over the row's own index map (S = len_b) in the fixed order of step 4 --
 * and +0.0 in every sample from len_b to max_samples.  The workspace stays dense, (rows, Tmax, Nr): hipfeat_grad_workspace_ragged is the
 * arithmetic of hipfeat_grad_workspace at T = Tmax.  h_lengths is a host array, checked and staged as for hipfeat_stft_run_ragged.  No
 * atomics, no memset: a row's gradient has the same bits alone, in any batch and under any piece size.  Statuses as for the uniform
 * twins, with max_samples in the place of num_samples; every refusal comes before any device call.
 */
HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_workspace_ragged(const hipfeat_grad* grad, int64_t batch, int64_t max_samples, const int64_t* h_lengths,
                                                                int64_t budget_bytes, int64_t* rows_per_piece, int64_t* floats);
HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_run_ragged(hipfeat_grad* grad, const float* d_wave, int64_t batch, int64_t max_samples, int64_t row_stride,
                                                          const int64_t* h_lengths, const float* d_grad_out, int64_t grad_out_floats,
                                                          const float* d_grad_log_energy, float* d_grad_wave, int64_t grad_wave_stride,
                                                          float* d_workspace, int64_t workspace_floats, void* stream);

/* ---- bulk save path: the per-batch host work of the offline driver ------------------------------- */
/*
 * What lhotse's _save_worker does per CUT in the interpreter behind compute_and_store_features_batch (lhotse/cut/set.py:2307-2363:
 * FeaturesWriter.write of one matrix -- lhotse/features/io.py:499-525 --, a Features object, validate_features, fastcopy(cut),
 * to_dict, json) is done per BATCH here, in plain host code that runs with the GIL released; no device is touched.
 *
 * hipfeat_archive_*: an append-only archive of feature rows striped over num_files flat files (1 = the single-file "hip_archive" of
 * lhotse_amd/storage.py).  hipfeat_archive_append writes the packed (sum h_num_frames, cols) matrix of one batch exactly as it left the
 * device (float32: bytes_per_value 4; binary16: 2): the batch is cut into num_files consecutive runs of whole cuts of about equal
 * bytes, run k is appended to file k by its own thread (writers to different files do not share an inode's page-cache locks);
 * h_file[b] / h_byte_offset[b] say where the rows of cut b begin.  The storage key of a cut is "<byte offset>:<rows>:<cols>[:f16]".
 *
 * hipfeat_manifest_lines: the JSONL lines of one batch.  Line b = head_b + mid[h_file[b]] + key_b + tail_b + "\n", where head_b / tail_b
 * are the two halves of the cut's own serialisation up to / from the storage fields (made by the caller where the cut was loaded --
 * lhotse's loader workers -- because they do not depend on the extraction), mid[k] = `<JSON-escaped path of file k>", "storage_key": "`
 * and key_b the key above.  heads / tails / mids are concatenated byte strings with (n + 1) int64 offsets each.  h_expected_frames
 * (optional; entries < 0 are skipped) is the frame count each manifest half states: a mismatch with h_num_frames is the frame-count
 * contract validate_features asserts (lhotse/qa.py:286-301) and fails the call before anything is written.  h_out needs
 * sum(len(head_b) + len(tail_b) + longest mid + 65) bytes; on "too small" *h_out_bytes holds that number.
 */
typedef struct hipfeat_archive hipfeat_archive;
HIPFEAT_API hipfeat_status hipfeat_archive_open(const char* const* h_paths, int32_t num_files, int32_t append, hipfeat_archive** archive);
HIPFEAT_API hipfeat_status hipfeat_archive_append(hipfeat_archive* archive, const void* h_matrix, int64_t batch, const int64_t* h_num_frames,
                                                  int32_t cols, int32_t bytes_per_value, int32_t* h_file, int64_t* h_byte_offset);
HIPFEAT_API int64_t hipfeat_archive_size(const hipfeat_archive* archive, int32_t file); /* bytes in file `file`, -1 if out of range */
HIPFEAT_API hipfeat_status hipfeat_archive_close(hipfeat_archive* archive);
HIPFEAT_API hipfeat_status hipfeat_manifest_lines(const char* h_heads, const int64_t* h_head_offsets, const char* h_tails,
                                                  const int64_t* h_tail_offsets, int64_t batch, const int64_t* h_num_frames,
                                                  const int64_t* h_expected_frames, const char* h_mids, const int64_t* h_mid_offsets,
                                                  int32_t num_files, const int32_t* h_file, const int64_t* h_byte_offset, int32_t cols,
                                                  int32_t bytes_per_value, char* h_out, int64_t out_capacity, int64_t* h_out_bytes);

/* ---- the offline driver's extraction step, one asynchronous call per batch of HOST waveforms -------------------- */
/*
 * Behind compute_and_store_features_batch the extractor is handed a list of host tensors per batch and its result goes to a save
 * thread (lhotse/cut/set.py:2365-2404).  A host pipeline does that step inside the library: hipfeat_host_pipeline_submit packs the
 * cuts (h_items[b] = pointer to h_num_samples[b] float32 samples, or int16 PCM when pcm16 != 0; pageable or page-locked) into
 * page-locked staging with `copy_threads` persistent host threads, and ENQUEUES, chunk by chunk on two private streams, the upload,
 * [hipfeat_pcm16_to_float,] the plan's feature launch (per-item reflect edges; zero_pad_batch != 0: edge_rule "batch_zero_pad"),
 * [hipfeat_float_to_half when half_out != 0] and the download into a page-locked result buffer owned by the pipeline.  It returns
 * without waiting for the device: *h_out is where the packed (*h_out_rows, feature_dim) matrix WILL be (float32, or binary16 with
 * half_out), h_num_frames[b] the frame counts (known at once), *ticket the handle.  hipfeat_host_pipeline_wait blocks until that
 * batch's features are in *h_out; hipfeat_host_pipeline_release gives the buffer back (after which *h_out may be overwritten by a later
 * batch).  Up to 64 results may be outstanding; submitting batch n + 1 before waiting for batch n is the point: its packing and
 * upload overlap batch n's download.  One pipeline per plan and calling thread; wait / release may come from another thread.
 */
typedef struct hipfeat_host_pipeline hipfeat_host_pipeline;
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_create(const hipfeat_plan* plan, int32_t copy_threads, hipfeat_host_pipeline** pipeline);
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_destroy(hipfeat_host_pipeline* pipeline);
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_submit(hipfeat_host_pipeline* pipeline, const void* const* h_items, const int64_t* h_num_samples,
                                                        int64_t batch, int32_t pcm16, int32_t zero_pad_batch, int32_t half_out,
                                                        int64_t* h_num_frames, void** h_out, int64_t* h_out_rows, int64_t* ticket);
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_wait(hipfeat_host_pipeline* pipeline, int64_t ticket);
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_release(hipfeat_host_pipeline* pipeline, int64_t ticket);
/* The pipeline thread's own clock since creation, h_stats[4] = {nanoseconds busy with batches, of those: packing into page-locked
 * staging, of those: waiting for a staging set's previous uploads / downloads (back-pressure from PCIe and the device), batches}:
 * lets a driver say which stage binds its run. */
HIPFEAT_API hipfeat_status hipfeat_host_pipeline_stats(const hipfeat_host_pipeline* pipeline, int64_t* h_stats);
/*
 * ABI v5: upload straight out of the loader's memory.  What lhotse's driver receives per batch is whatever its DataLoader delivered
 * (lhotse/cut/set.py:2374-2398): pageable arrays, which the pipeline above first copies into page-locked staging -- measured as the
 * largest single CPU consumer of the offline path once the loader keeps up (4-5 of 14 busy CPUs, profiles/r06_ring_loader_ab.txt).
 * hipfeat_host_register page-locks [ptr, ptr + bytes) of the CALLER's memory for DMA by `device` (any mapping: the slots of a
 * shared-memory ring that loader processes fill); hipfeat_host_unregister(ptr) undoes it (before the memory is unmapped; never while a
 * batch that reads it is outstanding).  hipfeat_host_pipeline_submit recognises a batch whose cuts all lie in ONE registered range, in
 * ascending order, each on a 16-byte boundary and (nearly) back to back, and uploads that span with one copy: no staging, no packing
 * threads.  Everything else about the call is unchanged (the cuts' memory must stay untouched until _wait returns, as before).
 * hipfeat_host_pipeline_direct_batches = how many batches of the pipeline went that way so far (-1: NULL pipeline).
 */
HIPFEAT_API hipfeat_status hipfeat_host_register(int32_t device, void* ptr, int64_t bytes);
HIPFEAT_API hipfeat_status hipfeat_host_unregister(void* ptr);
HIPFEAT_API int64_t hipfeat_host_pipeline_direct_batches(const hipfeat_host_pipeline* pipeline);

#ifdef __cplusplus
}
#endif
#endif /* HIPFEAT_H_ */
