/*
 * sylber_hip.h — C-ABI of libsylber_hip.so: the MI355X (gfx950) implementation of the SYLBER
 * Segmenter forward path.
 *
 * The reference has no FFI layer; its de-facto operator boundary is three Python call sites inside
 * Segmenter.__call__ (reference: sylber/model/sylber.py):
 *   (1) sylber.py:122   hidden = self.speech_model(batch, attention_mask=mask).last_hidden_state
 *                       (transformers.HubertModel, 9 layers)           -> sylber_forward()
 *   (2) sylber.py:126   get_segment(states, norm_threshold, merge_threshold)
 *                       (sylber/utils/segment_utils.py:72-131)         -> sylber_segment()
 *   (3) sylber.py:133   states[s:e].mean(0) per segment                -> sylber_segment() (fused)
 * and the weight hand-over at construction, sylber.py:41-54
 *   (HubertModel(config); load_state_dict(strict=False); eval().to(device)) -> sylber_create().
 *
 * Conventions: extern "C", opaque handle, int status (0 = ok, non-zero = error; text via
 * sylber_last_error()), no exceptions and no torch / HIP types in the signatures.  All *_dev
 * pointers are device pointers owned by the caller; `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Calls are stream-ordered and asynchronous.  A handle is bound to one
 * GPU and is not thread-safe; distinct handles are independent.
 */
#ifndef SYLBER_HIP_H
#define SYLBER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYLBER_MAX_LAYERS 12
#define SYLBER_HIDDEN 768
#define SYLBER_CONV_DIM 512

typedef struct sylber_ctx* sylber_t;

/* compute precision of the encoder GEMMs */
/* SYLBER_FP8 (BASELINE.json configs[4]): as SYLBER_BF16, but the four projection GEMMs around the attention (q/k/v, out) and the two FFN
 * GEMMs of every encoder layer (all of the encoder's weight GEMMs) run on OCP microscaling FP8 operands (e4m3 elements, one E8M0 power-of-two scale per 32 elements along K) through the
 * block-scaled gfx950 MFMA, fp32 accumulation; tolerance vs the bf16 mode is stated in tests/test_gpu_fp8.py */
/* SYLBER_FP16: exactly the SYLBER_BF16 path (same kernels, same matrix-pipe rate) with IEEE half as the 16-bit operand /
 * activation format: 10 instead of 7 mantissa bits at every hand-over, conversions saturate at +-65504 (measured agreement
 * with the fp32 reference: DESIGN.md) */
/* SYLBER_MIXED16: the conv stack as SYLBER_FP16 (that is where the bf16 mode makes its error: 13 hand-overs of O(1)
 * activations), the encoder as SYLBER_BF16; the feature-projection LayerNorm converts (measured cost / agreement: DESIGN.md) */
/* SYLBER_SPLIT16: every MFMA operand (activations and weights) is a PAIR of IEEE halves, hi = half(x) and lo = half(x - hi)
 * (22 significand bits), and every contraction is three fp16 MFMA passes into one fp32 accumulator (hi.hi + lo.hi + hi.lo);
 * erf GELU, fp32 residual stream / statistics as everywhere.  fp32-grade decisions (segment tables as the fp32 mode's)
 * at about three times the fp16 step instead of the fourteen times of SYLBER_FP32's f32 MFMA. */
enum { SYLBER_BF16 = 0, SYLBER_FP32 = 1, SYLBER_FP8 = 2, SYLBER_FP16 = 3, SYLBER_MIXED16 = 4, SYLBER_SPLIT16 = 5 };

/* HOST pointers to fp32 weights in the layout of HubertModel.state_dict().
 * Replaces the state_dict hand-over at sylber.py:51-54. */
typedef struct {
    const float* q_w; const float* q_b;       /* [768,768],[768] */
    const float* k_w; const float* k_b;
    const float* v_w; const float* v_b;
    const float* o_w; const float* o_b;
    const float* ln1_w; const float* ln1_b;   /* layer_norm */
    const float* ff1_w; const float* ff1_b;   /* intermediate_dense [3072,768],[3072] */
    const float* ff2_w; const float* ff2_b;   /* output_dense [768,3072],[768] */
    const float* ln2_w; const float* ln2_b;   /* final_layer_norm */
} SylberLayerWeights;

typedef struct {
    int32_t num_layers;                        /* encoding_layer, sylber.py:34 (default 9) */
    const float* conv_w[7];                    /* [512,1,10], 4x[512,512,3], 2x[512,512,2] */
    const float* gn_w; const float* gn_b;      /* conv_layers.0.layer_norm (GroupNorm affine) [512] */
    const float* fp_ln_w; const float* fp_ln_b;/* feature_projection.layer_norm [512] */
    const float* fp_w; const float* fp_b;      /* feature_projection.projection [768,512],[768] */
    const float* pos_w;                        /* EFFECTIVE pos-conv weight g*v/||v|| [768,48,128] */
    const float* pos_b;                        /* [768] */
    const float* enc_ln_w; const float* enc_ln_b;
    SylberLayerWeights layers[SYLBER_MAX_LAYERS];
} SylberWeights;

/* number of 50 Hz frames the 7-layer conv stack yields for n_samples (TP:664-677) */
int32_t sylber_num_frames(int32_t n_samples);
/* frame pitch per utterance of the library's internal activation buffers for a batch padded to n_samples (>= the
 * frame count, a multiple of 32); informational: workspace sizing and roofline byte counts */
int32_t sylber_padded_frames(int32_t n_samples);

/* copies + packs the weights onto `device` (bf16 MFMA layouts, conv taps interleaved) */
int sylber_create(const SylberWeights* w, int device, int precision, sylber_t* out);
void sylber_destroy(sylber_t h);
const char* sylber_last_error(void);

/* (1) waveform batch -> last_hidden_state.
 *   wav_dev      [B, Lmax] fp32, rows right-padded with zeros (sylber.py:99-117)
 *   lengths_host [B] valid samples per row (the attention_mask of sylber.py:104-118, run-length
 *                coded), or NULL for "all rows full" (identical numerics to an all-ones mask)
 *   hidden_dev   [B, T, 768] fp32, T = sylber_num_frames(Lmax); padded frames are computed and
 *                returned exactly like the reference does (sylber.py:125-135)
 */
int sylber_forward(sylber_t h, const float* wav_dev, const int32_t* lengths_host, int32_t B, int32_t Lmax,
                   float* hidden_dev, void* stream);
/* lengths_host is read before the call returns (the frame counts travel to the device as kernel arguments: no
 * pageable copy, no host synchronisation).  A handle is single-stream: it owns ONE workspace, so two forwards of the
 * same handle must be ordered on the same stream; use one handle per in-flight batch to overlap batches. */

/* (2)+(3) boundary detection + segment mean-pool, bit-exact w.r.t. the reference's numpy float32 evaluation order.
 * Round 6: frame norms, one workgroup per unbroken run of speech frames (independent instances of get_segment's two phases: a
 * non-speech frame resets the scan, segment_utils.py:84-90), compaction and pooling as four launches that use the whole chip
 * (SYLBER_OPT_SEGMENT = -1: the one-workgroup-per-utterance kernel of rounds 1-5).  Touches no encoder workspace, so it may run on a
 * side stream under the same handle's next sylber_forward; it does use a per-handle scratch slab (frame norms, slot table): the
 * sylber_segment calls of ONE handle must be ordered on one stream.
 *   hidden_dev [B, T, D] fp32 (D = 768 on the product path)
 *   seg_dev    [B, T, 2] int64  (start, end-exclusive) frame indices, first nseg_dev[b] rows valid
 *   nseg_dev   [B] int32
 *   feat_dev   [B, T, D] fp32 mean-pooled features, first nseg_dev[b] rows valid (may be NULL)
 */
int sylber_segment(sylber_t h, const float* hidden_dev, int32_t B, int32_t T, int32_t D, float norm_thr,
                   float merge_thr, int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream);
/* batch-invariant sibling of sylber_segment: row b is segmented and pooled as if it had exactly frames_host[b] frames
 * (get_segment(states[:frames_host[b]])): frames at or past that count are never read, a run of speech frames ends there as at the
 * end of an array, and every table entry lies in [0, frames_host[b]).  frames_host [B] in [1, T], read before the call returns (the
 * counts travel as kernel arguments).  Buffers and pitch (T) as sylber_segment.  Wide path only: refused under
 * SYLBER_OPT_SEGMENT = -1. */
int sylber_segment_frames(sylber_t h, const float* hidden_dev, const int32_t* frames_host, int32_t B, int32_t T, int32_t D,
                          float norm_thr, float merge_thr, int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream);

/* ---- packed variable-length batches ------------------------------------------------------------
 * A ragged batch without padding to its longest clip: clip b gets a slot of frames at frame offset offsets[b], the slots follow each
 * other, and the whole batch runs as one pseudo-utterance of offsets[B] frames.  Per clip the results are bit-identical to
 * sylber_forward with SYLBER_OPT_PER_UTTERANCE = 1 (and to that clip alone) and to sylber_segment_frames.  Host only, no GPU:
 *   samples_host [B] samples per clip, each >= 400 (one frame)
 *   offsets      [B + 1] out: slot b = frames [offsets[b], offsets[b + 1]), offsets[0] = 0, offsets[B] = the batch's total frames.  A slot
 *                holds every conv layer's valid rows of a call of the clip's own length, rounded up to a multiple of 64 frames (whole
 *                attention key tiles), so it is 1 to 65 frames longer than frames[b]
 *   frames       [B] out: sylber_num_frames(samples_host[b])
 * Fails (status 1) on B < 1, a clip below 400 samples, or a batch whose waveform (320 x offsets[B] samples) exceeds 2^31 - 1 samples. */
int sylber_packed_layout(const int32_t* samples_host, int32_t B, int32_t* offsets, int32_t* frames);
/* (1) for a packed batch.  wav_dev: 320 x offsets[B] fp32 samples, clip b's samples_host[b] samples from sample 320 x offsets[b], zeros
 * to the end of its slot.  hidden_dev [offsets[B], 768] fp32: clip b's hidden states are rows [offsets[b], offsets[b] + frames[b]); the
 * rows behind them hold whatever the forward computes there.  SYLBER_BF16 and SYLBER_FP16 only; refused in graph mode, with a stop
 * stage, SYLBER_OPT_CONV0_VALU or SYLBER_OPT_ATTN_QUERIES_PER_WAVE set.  The slot tables travel as kernel arguments (no host copy);
 * samples_host is read before the call returns.  Same workspace and stream rules as sylber_forward. */
int sylber_forward_packed(sylber_t h, const float* wav_dev, const int32_t* samples_host, int32_t B, float* hidden_dev, void* stream);
/* (2)+(3) for a packed batch: clip b is segmented and pooled as sylber_segment_frames segments hidden[offsets[b] : offsets[b] + frames[b]]
 * alone.  Tables relative to the clip's first frame, kcap = max frames[b] slots per clip: seg_dev [B, kcap, 2], nseg_dev [B], feat_dev
 * [B, kcap, 768] or NULL.  Refused under SYLBER_OPT_SEGMENT = -1. */
int sylber_segment_packed(sylber_t h, const float* hidden_dev, const int32_t* samples_host, int32_t B, float norm_thr, float merge_thr,
                          int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream);
/* each clip's own hidden states of a packed batch, back to back: out_dev [sum frames[b], 768] fp32 (clip b from row frames[0] + ... +
 * frames[b - 1]), from sylber_forward_packed's hidden_dev.  No handle, stream-ordered; one device-to-host copy then fetches them all. */
int sylber_packed_gather(const float* hidden_dev, const int32_t* samples_host, int32_t B, float* out_dev, void* stream);

/* ---- file ingest on the device (replaces sylber.py:83-86) -------------------
 *   wav, sr = torchaudio.load(file); if sr != 16000: wav = torchaudio.transforms.Resample(sr, 16000)(wav);
 *   wav = (wav - wav.mean()) / wav.std()
 * pcm_dev      interleaved little-endian PCM frames as they sit in the file's data chunk, on the device
 * sample_width bytes per sample: 1 (uint8), 2 (int16), 3 (int24), 4 (int32), scaled to [-1, 1) like torchaudio.load;
 *              -4 / -8: IEEE float32 / float64 samples (WAVE_FORMAT_IEEE_FLOAT), taken as they are
 * normalize    non-zero: (x - mean) / unbiased std over all channels x frames
 * wav_out_dev  [channels, sylber_ingest_num_frames(frames_in, sr_in)] fp32, every channel one future batch row
 * workspace_dev sylber_ingest_workspace_bytes(sr_in) bytes, 8-byte aligned, owned by the caller
 * Stateless (no handle); stream-ordered.  Resampler: torchaudio's sinc_interp_hann defaults (csrc/ingest.hip). */
int64_t sylber_ingest_num_frames(int64_t frames_in, int32_t sr_in);
int64_t sylber_ingest_workspace_bytes(int32_t sr_in);
int sylber_ingest(const void* pcm_dev, int32_t sample_width, int32_t channels, int64_t frames_in, int32_t sr_in,
                  int32_t normalize, float* wav_out_dev, void* workspace_dev, void* stream);

/* FLAC container -> interleaved integer PCM on the HOST (torchaudio.load at sylber.py:83 decodes .flac files too; the reference's data code falls back from .wav to
 * .flac, sylber/dataset/collective_audio_segment.py:61-67).  A FLAC stream is a serial bit-granular entropy code: host work, like the RIFF header parse; the decoded
 * samples then go through sylber_ingest as 16- or 32-bit PCM scaled to full range.  data = the whole file in memory (an ID3v2 tag in front is skipped).
 * sylber_flac_info: sample rate, channels, bits per sample (4..32), frames (0 = the encoder did not know).  sylber_flac_decode: out_host [capacity_frames][channels] int32 at
 * the samples' own scale, or NULL to verify and count only; every frame's CRC-8 / CRC-16 is checked and, when STREAMINFO carries the encoder's MD5 of the unencoded audio,
 * the decoded PCM against it.  Stateless, no device is touched.  Parity unpinned (no codec / FLAC file in the build image): csrc/flac_host.hip restates RFC 9639. */
int sylber_flac_info(const uint8_t* data_host, int64_t size, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample, int64_t* frames);
int sylber_flac_decode(const uint8_t* data_host, int64_t size, int32_t* out_host, int64_t capacity_frames, int64_t* frames_out);

/* ---- the two callers right behind the path, on device-resident outputs of sylber_segment --- */
/* N4: k-means tokenisation, KMQuantizer.get_indices (sylber/model/quantizer.py:86-111; codebook look-up of
 * vector_quantize_pytorch's EuclideanCodebook: argmin_c ||x - c||, first index on ties).
 *   feats_dev [n, D] fp32 (D % 16 == 0), centroids_dev [K, D] fp32, normalize != 0: x / sqrt(sum x^2 + 1e-8) * 6 first
 *   idx_dev [n] int32; workspace_dev: sylber_km_workspace_floats(n, K, D) floats.  Exact-fp32 contraction.
 *   Ids are always in [0, K): a NaN score is never chosen, and a row whose scores are all NaN (a NaN or inf - inf token) gets id 0,
 *   upstream's argmax of an all-NaN row.  The same holds for sylber_km_assign_residual and sylber_rvq_assign.  (sylber_kmeans_assign
 *   differs on purpose: such a row gets 2147483647 there, "no nearest centroid", which the inverted-file indexes read as "in no list".)
 *   K < 4 with K % 4 != 0 is refused. */
int64_t sylber_km_workspace_floats(int32_t n, int32_t K, int32_t D);
int sylber_km_assign(const float* feats_dev, int32_t n, const float* centroids_dev, int32_t K, int32_t D, int32_t normalize,
                     int32_t* idx_dev, float* workspace_dev, void* stream);
/* KMQuantizer.decode (quantizer.py:127-133): out[r] = centroids[clip(idx[r], 0)] */
int sylber_km_decode(const int32_t* idx_dev, int32_t n, const float* centroids_dev, int32_t K, int32_t D, float* out_dev, void* stream);

/* ResidualKMQuantizer.get_indices (quantizer.py:137-160): stage 1 = sylber_km_assign(c1, normalize 0) into idx_dev[r][0], then
 * r = x - c1[max(idx1, 0)] (one fp32 subtract per element, token - z_q) assigned against c2 into idx_dev[r][1].
 *   idx_dev [n, 2] int32; workspace_dev: sylber_km_residual_workspace_floats(n, K1, K2, D) floats */
int64_t sylber_km_residual_workspace_floats(int32_t n, int32_t K1, int32_t K2, int32_t D);
int sylber_km_assign_residual(const float* feats_dev, int32_t n, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2,
                              int32_t D, int32_t* idx_dev, float* workspace_dev, void* stream);
/* ResidualKMQuantizer.decode (quantizer.py:174-178): out[r] = c1[max(idx[r][0], 0)] + c2[max(idx[r][1], 0)] (z_q1 + z_q2) */
int sylber_km_decode_residual(const int32_t* idx_dev, int32_t n, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2,
                              int32_t D, float* out_dev, void* stream);

/* Fitting k-means unit codebooks (sylber_amd/kmeans.py: fit_kmeans and the quantizers it returns).  Device pointers, exact fp32
 * contractions, results independent of the launch geometry.
 * sylber_km_normalize: y[r] = x[r] / sqrt(sum x[r]^2 + 1e-8) * 6, the arithmetic of sylber_km_assign's normalize (y may not alias x).
 * sylber_kmeans_assign: idx_dev[r] = argmin_k fmaf(-2, x_r . c_k, ||c_k||^2), ties to the smallest k -- the bits of sylber_km_assign
 *   for every K >= 1 -- without materialising the [n, K] dot matrix.  Optional outputs (nullable): dmin_dev [n] the minimum itself,
 *   inertia_dev (one double) = sum_r max(0, ||x_r||^2 + dmin[r]) summed in fp64 in a fixed order, changed_dev (one int64) = rows whose
 *   label differs from prev_idx_dev [n].  x_dev [n, D], c_dev [K, D] fp32, D % 16 == 0;
 *   workspace_dev: sylber_kmeans_assign_workspace_floats(n, K, D) floats (O(n + K)).
 * sylber_kmeans_update: counts_dev[k] = rows with idx_dev == k; for every k with counts > 0, c_dev[k] = fp32(fp64 sum of its rows /
 *   count), the sum taken over the rows in ascending order in pieces of 512 rows, the pieces added left to right; clusters without
 *   rows keep c_dev[k].  order_dev [n] int64: the row indices grouped by label in ascending label order, ascending within a label
 *   (a stable sort of idx_dev).  workspace_dev: sylber_kmeans_update_workspace_bytes(n, K, D) bytes.
 * sylber_kmeans_seed: k-means++ (one candidate per step) over x_dev [n, D], D % 4 == 0, with u_dev [K] fp64 uniforms in [0, 1):
 *   chosen[0] = floor(u[0] n); after each center, dist[r] = min(dist[r], sum_j (x_rj - c_j)^2) (fmaf chain in ascending j), and the
 *   next center is the first r whose fp64 prefix sum of dist (256-row block sums, each the last element of an inclusive in-block
 *   scan, prefixed across blocks) exceeds u[j] * total.  chosen_dev [K] int32.  Asynchronous: status_dev (one int32) is 0 when done,
 *   1 when the rows have fewer than K distinct values (total == 0).  workspace_dev: sylber_kmeans_seed_workspace_floats(n) floats. */
int sylber_km_normalize(const float* x_dev, int32_t n, int32_t D, float* y_dev, void* stream);
int64_t sylber_kmeans_assign_workspace_floats(int32_t n, int32_t K, int32_t D);
int sylber_kmeans_assign(const float* x_dev, int32_t n, const float* c_dev, int32_t K, int32_t D, int32_t* idx_dev, float* dmin_dev,
                         double* inertia_dev, const int32_t* prev_idx_dev, int64_t* changed_dev, float* workspace_dev, void* stream);
int64_t sylber_kmeans_update_workspace_bytes(int32_t n, int32_t K, int32_t D);
int sylber_kmeans_update(const float* x_dev, int32_t n, int32_t D, const int32_t* idx_dev, const int64_t* order_dev, int32_t K,
                         float* c_dev, int32_t* counts_dev, void* workspace_dev, void* stream);
int64_t sylber_kmeans_seed_workspace_floats(int32_t n);
int sylber_kmeans_seed(const float* x_dev, int32_t n, int32_t D, int32_t K, const double* u_dev, int32_t* chosen_dev,
                       int32_t* status_dev, float* workspace_dev, void* stream);

/* Exact k-nearest-neighbour search (sylber_amd/search.py: SyllableIndex).  Device pointers, exact fp32, results independent of the
 * launch geometry, the split count and how the queries are chunked.
 * sylber_knn_search: for each query row i of q_dev [n, D] the k best database rows j of db_dev [N, D] (D % 16 == 0, N < 2^31,
 *   1 <= k <= 128) under the score s(i, j) = fmaf(-2, q_i . x_j, c_j), the dot product the exact-fp32 contraction of
 *   sylber_kmeans_assign (ascending k, one rounding per product).  metric SYLBER_KNN_L2: c_j = db_norm_dev[j] (sylber_knn_row_norms);
 *   SYLBER_KNN_IP: c_j = 0 (db_norm_dev ignored; cosine = IP on sylber_knn_unit_rows).  Each list is ordered by (s, j) ascending: the
 *   smaller score, then the smaller j.  A candidate with a NaN score is never returned; with q_group_dev [n] and db_group_dev [N]
 *   (int32, both or neither) a candidate with db_group[j] == q_group[i] is skipped.  Rows with fewer than k admissible candidates
 *   end in idx -1 / score +inf.  Reported scores: L2 max(0, ||q_i||^2 + s) with ||q_i||^2 as sylber_knn_row_norms (fp32; for k = 1
 *   idx is sylber_kmeans_assign's label and the score max(0, ||q||^2 + dmin)); IP the dot product -s / 2, exact.  score_dev [n, k]
 *   fp32, idx_dev [n, k] int64.  splits: database splits S (0 = automatic: enough workgroups to cover the chip; any other value is
 *   clamped to [1, ceil(N / 128)]).  workspace_dev: sylber_knn_workspace_bytes(n, N, D, k, splits) bytes, O(n S k); no [n, N] buffer.
 * sylber_knn_splits: the S that a call with these n, N and splits uses.
 * sylber_knn_row_norms: out[r] = sum_c x[r][c]^2, the fmaf chain of sylber_kmeans_assign's norms (lane c % 64 over ascending c, then
 *   the wave butterfly).
 * sylber_knn_unit_rows: y[r] = x[r] / sqrtf(that sum), rows whose sum is 0 stay 0 (y may not alias x). */
enum { SYLBER_KNN_L2 = 0, SYLBER_KNN_IP = 1 };
int32_t sylber_knn_splits(int32_t n, int32_t N, int32_t splits);
int64_t sylber_knn_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t k, int32_t splits);
int sylber_knn_row_norms(const float* x_dev, int32_t n, int32_t D, float* out_dev, void* stream);
int sylber_knn_unit_rows(const float* x_dev, int32_t n, int32_t D, float* y_dev, void* stream);
int sylber_knn_search(const float* q_dev, int32_t n, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev, int32_t metric,
                      int32_t k, const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits, float* score_dev,
                      int64_t* idx_dev, void* workspace_dev, void* stream);

/* Two-stage search (sylber_amd/search.py: SyllableIndex.search_refined): a 16-bit MFMA scan picks m candidates per query, the exact
 * score of sylber_knn_search re-ranks them.  The result is sylber_knn_search restricted to the candidates; with m >= N it is
 * sylber_knn_search bit for bit.
 * sylber_knn16_pack: out16_dev [n, D] = the fp32 rows x_dev [n, D] (D % 16 == 0) rounded to nearest even to IEEE half
 *   (SYLBER_KNN16_FP16) or bfloat16 (SYLBER_KNN16_BF16); NaN stays NaN.  fp16 saturates at +-65504, and *sat_count_dev (int32 on the
 *   device, may be null; the caller zeroes it) grows by the number of FINITE values beyond +-65504.
 * sylber_knn16_scan: candidates of query i = the m best database rows (1 <= m <= 128) under the strict order (t, j) of the coarse
 *   score t(i, j) = fmaf(-2, dot16(q16_i, x16_j), c_j): dot16 the fp32-accumulated sum of the exact 16-bit products in the one
 *   fixed order of the kernel's MFMA chain (ascending K), c_j = db_norm_dev[j] (the fp32 norms of sylber_knn_search) or 0 when
 *   db_norm_dev is null.  NaN t and (with both group arrays) rows of the query's group are not admissible.  cand_dev [n, m] int32,
 *   best first, padded with -1: bitwise independent of splits, of how the queries are chunked and of what the workspace held.
 *   workspace_dev: sylber_knn16_workspace_bytes(n, N, D, m, splits) bytes; splits as sylber_knn_search.
 * sylber_knn_rerank: for each candidate j of cand_dev [n, m] (-1 = none) the score s = fmaf(-2, q_i . x_j, c_j) with the bits of
 *   sylber_knn_search (the ascending fmaf chain from 0); NaN s dropped; ordered by (s, j), the best k (1 <= k <= m) reported as
 *   sylber_knn_search reports them (L2 max(0, ||q_i||^2 + s), IP -s / 2, padding idx -1 / score +inf). */
enum { SYLBER_KNN16_FP16 = 0, SYLBER_KNN16_BF16 = 1 };
int sylber_knn16_pack(const float* x_dev, int32_t n, int32_t D, int32_t storage, void* out16_dev, int32_t* sat_count_dev, void* stream);
int64_t sylber_knn16_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t m, int32_t splits);
int sylber_knn16_scan(const void* q16_dev, int32_t n, const void* db16_dev, int32_t N, int32_t D, const float* db_norm_dev,
                      int32_t storage, int32_t m, const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits,
                      int32_t* cand_dev, void* workspace_dev, void* stream);
int sylber_knn_rerank(const float* q_dev, int32_t n, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev, int32_t metric,
                      const int32_t* cand_dev, int32_t m, int32_t k, float* score_dev, int64_t* idx_dev, void* stream);

/* Product-quantized search (sylber_amd/pq.py: PQSyllableIndex): a row of D floats is stored as M bytes (1 <= M <= 64, D % M == 0,
 * dsub = D / M a multiple of 16), byte m the nearest of the 256 centroids cb_dev [M, 256, dsub] of sub-space m (columns
 * [m dsub, (m + 1) dsub)); cnorm_dev [M, 256] = sylber_knn_row_norms of the centroids.
 * sylber_pq_encode: code_dev [n, M] = for every m the label sylber_kmeans_assign gives the sub-row against codebook m, bit for bit:
 *   argmin_c fmaf(-2, x . c, ||c||^2), the dot product the ascending fmaf chain from 0, ties to the smaller c; all M sub-spaces in one
 *   launch.  A sub-row without a comparable distance (it holds a NaN) gets code 0, and bad_dev [n] is 1 for such a row, else 0.
 * sylber_pq_decode: out_dev [n, D] = the centroids the codes name.
 * sylber_pq_lut: lut_dev [n, M, 256], lut[i][m][c] = fmaf(-2, q_i[sub-row m] . cb[m][c], cm), the same chain; cm = cnorm[m][c]
 *   (SYLBER_KNN_L2) or 0 (SYLBER_KNN_IP: cnorm_dev may be null).
 * sylber_pq_scan: t(i, j) = ((lut[i][0][code[j][0]] + lut[i][1][code[j][1]]) + ...) + lut[i][M-1][code[j][M-1]], fp32 adds in ascending
 *   m.  The candidates of query i are the m best admissible rows under the strict order (t, j): t_dev / cand_dev [n, m], best first,
 *   padded with (+inf, -1).  A NaN t, a row with bad_dev[j] != 0 (bad_dev may be null: no mask) and, with both group arrays, a row
 *   of the query's group are not admissible.  Bitwise independent of splits (0 = automatic), of how the queries are chunked or
 *   share workgroups, and of what the workspace held.  workspace_dev: sylber_pq_workspace_bytes(n, N, M, m, splits) bytes; code_dev
 *   16-byte aligned. */
int sylber_pq_encode(const float* x_dev, int32_t n, int32_t D, const float* cb_dev, const float* cnorm_dev, int32_t M, uint8_t* code_dev,
                     uint8_t* bad_dev, void* stream);
int sylber_pq_decode(const uint8_t* code_dev, int32_t n, const float* cb_dev, int32_t M, int32_t D, float* out_dev, void* stream);
int sylber_pq_lut(const float* q_dev, int32_t n, int32_t D, const float* cb_dev, const float* cnorm_dev, int32_t M, int32_t metric,
                  float* lut_dev, void* stream);
int64_t sylber_pq_workspace_bytes(int32_t n, int32_t N, int32_t M, int32_t m, int32_t splits);
int sylber_pq_scan(const float* lut_dev, int32_t n, const uint8_t* code_dev, const uint8_t* bad_dev, int32_t N, int32_t M, int32_t m,
                   const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits, float* t_dev, int32_t* cand_dev,
                   void* workspace_dev, void* stream);

/* Inverted-file search (sylber_amd/search.py: IVFSyllableIndex): sylber_knn_search restricted, per query, to the rows of the lists it
 * probes.  The rows lie list by list in rows_dev (list l = positions list_offsets[l] .. list_offsets[l + 1], ascending original id
 * within a list); row_id_dev [N] maps a position to the row's original id, row_norm_dev / row_group_dev are in position order too.
 * sylber_ivf_work_items (host only, no GPU): the work items of one call.  pair_counts_host [nlist]: how many (query, probe slot)
 *   pairs probe each list; list_offsets_host [nlist + 1].  One item per (probed list, block of up to 128 of its pairs, cut of at
 *   most T of its 128-row tiles), in list order, 8 int32 each: {list, pair_begin, pair_count, row_lo, row_hi, cut, last, tile_begin};
 *   pair_begin indexes the pairs grouped by list, [row_lo, row_hi) are positions, last marks a list's final cut.  item_tiles: T
 *   (0 = automatic; raised where a list would need more than 16 cuts).  A probed empty list gets one item without rows.  Returns the
 *   number of items (-1: bad argument, or more than capacity); writes them when items_host is non-null and *cuts_out = the largest
 *   number of cuts of any probed list.
 * sylber_ivf_search: q_dev [n, D]; pair_dev [n * nprobe] int32: the flat indices (query * nprobe + slot) of the probe table grouped
 *   by list (a stable sort of the table by list id), every index exactly once; items_dev [n_items][8] as above for these pairs.
 *   Each pair's partial top-k lists (one per cut) hold (s, original id) with s = fmaf(-2, q . x, c) exactly as sylber_knn_search;
 *   the nprobe * cuts lists of a query are merged and reported as sylber_knn_search does (order (s, id), NaN never returned, group
 *   exclusion, -1 / +inf padding).  workspace_dev: sylber_ivf_workspace_bytes(n, nprobe, k, cuts) bytes, O(n nprobe cuts k). */
int32_t sylber_ivf_work_items(const int32_t* pair_counts_host, const int32_t* list_offsets_host, int32_t nlist, int32_t item_tiles,
                              int32_t* items_host, int32_t capacity, int32_t* cuts_out);
int64_t sylber_ivf_workspace_bytes(int32_t n, int32_t nprobe, int32_t k, int32_t cuts);
int sylber_ivf_search(const float* q_dev, int32_t n, int32_t D, int32_t nprobe, const int32_t* pair_dev, const int32_t* items_dev,
                      int32_t n_items, int32_t cuts, const float* rows_dev, const int32_t* row_id_dev, const float* row_norm_dev,
                      int32_t metric, int32_t k, const int32_t* q_group_dev, const int32_t* row_group_dev, float* score_dev,
                      int64_t* idx_dev, void* workspace_dev, void* stream);

/* Compressed inverted-file search (sylber_amd/pq.py: IVFPQSyllableIndex): sylber_pq_scan restricted, per query, to the rows of the
 * lists it probes.  The codes lie list by list in code_dev [N_listed, M] (list l = positions list_offsets_dev[l] ..
 * list_offsets_dev[l + 1], ascending original id within a list; 16-byte aligned); row_id_dev [N_listed] maps a position to the row's
 * original id; bad_dev (may be null: no mask) and row_group_dev are in position order too.  The codes are those of the rows
 * themselves (sylber_pq_encode), not of residuals, so lut_dev [n, M, 256] is sylber_pq_lut's table: one per query for all its lists.
 * sylber_ivfpq_scan: probe_dev [n, nprobe] int32 names the lists of each query (1 <= nprobe <= 128; an entry outside [0, nlist) names
 *   none).  t(i, j) is sylber_pq_scan's sum.  The candidates of query i are the m best (1 <= m <= 128) admissible rows of its lists
 *   under the strict order (t, original id): t_dev / cand_dev [n, m] (original ids), best first, padded with (+inf, -1).  A NaN t, a
 *   masked row and, with both group arrays, a row of the query's group are not admissible.  With every list probed the result is
 *   sylber_pq_scan's on the same rows, bit for bit.  Bitwise independent of splits (0 = automatic: about 512 workgroups, at most
 *   nprobe per query), of how the queries are chunked and of what the workspace held.  No host work: one workgroup per (query, split
 *   of its probe slots) reads the lists' bounds on the device.  workspace_dev: sylber_ivfpq_workspace_bytes(n, nprobe, m, splits)
 *   bytes (-1 for arguments that sylber_ivfpq_scan refuses). */
int64_t sylber_ivfpq_workspace_bytes(int32_t n, int32_t nprobe, int32_t m, int32_t splits);
int sylber_ivfpq_scan(const float* lut_dev, int32_t n, const int32_t* probe_dev, int32_t nprobe, const int32_t* list_offsets_dev,
                      int32_t nlist, const uint8_t* code_dev, const uint8_t* bad_dev, const int32_t* row_id_dev, int32_t N_listed, int32_t M,
                      int32_t m, const int32_t* q_group_dev, const int32_t* row_group_dev, int32_t splits, float* t_dev, int32_t* cand_dev,
                      void* workspace_dev, void* stream);

/* Residual codes (IVFPQSyllableIndex.build(..., residual=True)): a row's code is sylber_pq_encode's of r_j = x_j - centroid[l_j], l_j
 * its list, so the reconstruction is xhat_j = centroid[l_j] + (the centroids the code names), one fp32 addition per element.  The
 * table stays one per query: sylber_pq_lut's inner-product table (SYLBER_KNN_IP) for both metrics; what depends on the list and on
 * the row is added per row.  centroid_dev [nlist, D]; a list id outside [0, nlist) names no list.
 * sylber_ivfpq_list_terms: list_term_dev [n, nprobe], a[i][s] = -2 (q_i . centroid[probe[i][s]]), the dot product the ascending fmaf
 *   chain from 0 of sylber_knn_rerank; 0 for a slot that names no list.
 * sylber_ivfpq_recon_norms: nrm_dev [n] = ||xhat_j||^2 of the rows with codes code_dev [n, M] and lists list_dev [n]: the chain
 *   nrm = fmaf(xhat[e], xhat[e], nrm) from 0 in ascending e, one thread per row, so the bits are a function of the row alone.  A row
 *   in no list takes xhat = the centroids its code names.
 * sylber_ivfpq_decode: out_dev [n, D] = xhat of the same arguments.
 * sylber_ivfpq_scan_residual: sylber_ivfpq_scan with t(i, j) = (u + a[i][s]) + nrm_j, u sylber_pq_scan's sum, s the probe slot whose
 *   list holds the row and nrm_j = row_term_dev [N_listed] at the row's position (null: t = u + a[i][s]); both are added before the
 *   threshold test.  A row is in one list, so t's bits are a function of (query, row) alone.  Everything else, the workspace
 *   included, is sylber_ivfpq_scan's. */
int sylber_ivfpq_list_terms(const float* q_dev, int32_t n, int32_t D, const float* centroid_dev, int32_t nlist, const int32_t* probe_dev,
                            int32_t nprobe, float* list_term_dev, void* stream);
int sylber_ivfpq_recon_norms(const uint8_t* code_dev, int32_t n, const int32_t* list_dev, const float* centroid_dev, int32_t nlist,
                             const float* cb_dev, int32_t M, int32_t D, float* nrm_dev, void* stream);
int sylber_ivfpq_decode(const uint8_t* code_dev, int32_t n, const int32_t* list_dev, const float* centroid_dev, int32_t nlist,
                        const float* cb_dev, int32_t M, int32_t D, float* out_dev, void* stream);
int sylber_ivfpq_scan_residual(const float* lut_dev, int32_t n, const int32_t* probe_dev, int32_t nprobe, const int32_t* list_offsets_dev,
                               int32_t nlist, const uint8_t* code_dev, const uint8_t* bad_dev, const int32_t* row_id_dev, int32_t N_listed,
                               int32_t M, int32_t m, const int32_t* q_group_dev, const int32_t* row_group_dev, int32_t splits,
                               const float* list_term_dev, const float* row_term_dev, float* t_dev, int32_t* cand_dev,
                               void* workspace_dev, void* stream);

/* Phrase search (sylber_amd/search.py: SyllableIndex.search_phrases): query-by-example subsequence DTW of syllable sequences
 * (phrases, 1 <= m <= 64 rows) against every sequence of the database (runs of consecutive rows, at most 65 536 rows each).
 * Local cost of phrase row i against database row j, in fp32, from the score s = fmaf(-2, q_i . x_j, c_j) of sylber_knn_search
 * (same contraction, same bits):
 *   SYLBER_KNN_L2: d = max(0, ||q_i||^2 + s) with ||q_i||^2 as sylber_knn_row_norms, i.e. exactly the score sylber_knn_search reports;
 *   SYLBER_KNN_IP (cosine: phrase rows made unit rows as for sylber_knn_search): d = max(0, 1 - (-s / 2)) (the halving is exact, the
 *   subtraction rounds once);  a NaN d (a NaN row on either side) counts as +inf.
 * Subsequence DTW of a phrase of m rows against a sequence with columns j = 0 .. L - 1 (the phrase is consumed whole, its span in the
 * sequence is free), all additions in fp32, one per cell:
 *   A[0][j] = d[0][j]                                   start[0][j] = j
 *   A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      (terms outside the sequence are +inf)
 *             on equal values the predecessor is taken in that order: diagonal, then (i-1, j), then (i, j-1);
 *             start[i][j] = start of the predecessor taken
 *   cost = min_j A[m-1][j], the smallest such j on ties = end;   span = (row of start[m-1][end], row of end + 1)
 * A sequence whose cost is +inf is never returned.  Each phrase's list is ordered by (cost, sequence number) ascending, the strict
 * order sylber_knn_search uses; lists with fewer than k admissible sequences end in cost +inf, sequence -1, span (-1, -1).  Because
 * fp32 + and min in a fixed cell order are deterministic, the result is unique: it does not depend on the split of the database, the
 * packing or chunking of phrases, stale workspace contents, or whether the index came from one add or many.  m > L is legal
 * (vertical steps).  No normalisation by path length.
 * sylber_dtw_plan (host only, no GPU): seq_offsets_host [n_seq + 1] (first 0, ascending, last N: sequence s = rows offsets[s] ..
 *   offsets[s + 1]), phrase_len_host [n_phrases].  Packs the phrases, in order, into query blocks of 128 rows -- a phrase lies inside
 *   one 64-row half of one block; a block holds at most min(128, 4096 / k) phrases, fewer with block_phrases > 0 -- and cuts the
 *   database at sequence starts only: cut c begins at the first sequence start at or after row c N / C' (C' = splits, or automatic
 *   with splits = 0: enough workgroups to cover the chip, about 4 tiles of 128 rows or more each; at most 65 535), equal boundaries
 *   collapsing.  Returns the number of cuts C; writes cut_rows_host [C + 1] (cut c = rows cut_rows[c] .. cut_rows[c + 1]; needs
 *   cut_capacity >= C + 1) and phrase_row_host [n_phrases] (block * 128 + first row in the block) where non-null, *blocks_out and
 *   *block_phrases_out (the cap used).  Errors: -1 bad argument or capacity, -2 a phrase length outside [1, 64], -3 a sequence
 *   longer than 65 536 rows, -4 malformed offsets.
 * sylber_dtw_search: q_dev [n_blocks * 128, D] the phrase rows as packed by the plan (padding rows zero; unit rows for cosine);
 *   row_meta_dev [n_blocks * 128] int32: -1 for padding, else (row within its phrase) | (last row of its phrase) << 7 | (slot of its
 *   phrase in the block) << 8; slot_phrase_dev [n_blocks * 128]: the phrase number of each slot of each block, -1 behind the last;
 *   block_rows_dev [n_blocks]: rows in use; block_phrases: the largest number of slots of any block.  seq_id_dev [N]: the sequence
 *   of every row; cut_rows_dev [cuts + 1].  With phrase_group_dev [n_phrases] and seq_group_dev [n_seq] (both or neither) a sequence
 *   whose group equals the phrase's is skipped.  cost_dev [n_phrases, k] fp32, seq_dev [n_phrases, k] int64, span_dev
 *   [n_phrases, k, 2] int64 (first row, one past the last row).  At most one match per sequence: its best one.  workspace_dev:
 *   sylber_dtw_workspace_bytes(n_blocks, n_phrases, k, cuts) bytes, O(P C k); no [rows, N] buffer. */
int32_t sylber_dtw_plan(const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* phrase_len_host, int32_t n_phrases, int32_t k,
                        int32_t splits, int32_t block_phrases, int32_t* cut_rows_host, int32_t cut_capacity, int32_t* phrase_row_host,
                        int32_t* blocks_out, int32_t* block_phrases_out);
int64_t sylber_dtw_workspace_bytes(int32_t n_blocks, int32_t n_phrases, int32_t k, int32_t cuts);
int sylber_dtw_search(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                      const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N, int32_t D,
                      const float* db_norm_dev, int32_t metric, int32_t k, const int32_t* seq_id_dev, const int32_t* cut_rows_dev,
                      int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev, float* cost_dev, int64_t* seq_dev,
                      int64_t* span_dev, void* workspace_dev, void* stream);

/* Two-stage phrase search (sylber_amd/search.py: SyllableIndex.search_phrases_refined): a 16-bit MFMA subsequence-DTW scan picks m
 * candidate sequences per phrase, the exact subsequence DTW of sylber_dtw_search re-ranks them.  The result is sylber_dtw_search
 * restricted to the candidate sequences; with m at least the number of admissible sequences of finite cost it is sylber_dtw_search
 * bit for bit.  sylber_dtw_plan is called with m in place of k, so that a block's phrases fit the scan's lists.
 * sylber_dtw16_scan: q16_dev [n_blocks * 128, D] the packed phrase rows of sylber_dtw_search as sylber_knn16_pack rounds them,
 *   db16_dev [N, D] the database's 16-bit plane (both in `storage`); row_meta_dev, slot_phrase_dev, block_rows_dev, block_phrases,
 *   seq_id_dev, cut_rows_dev, cuts and the two group arrays as for sylber_dtw_search.  Coarse score t(i, j) = fmaf(-2,
 *   dot16(q16_i, x16_j), c_j) as sylber_knn16_scan's (c_j = db_norm_dev[j] under L2, 0 under IP); local cost in fp32
 *   L2: max(0, q_norm_dev[i] + t) with q_norm_dev [n_blocks * 128] = sylber_knn_row_norms of the UNROUNDED packed fp32 rows,
 *   IP: max(0, 1 - (0 - t / 2)); NaN counts as +inf.  Over these the recurrence of sylber_dtw_search; coarse cost of (phrase,
 *   sequence) = min_j A[m-1][j].  Candidates of a phrase = its m best (1 <= m <= 128) admissible sequences under (coarse cost,
 *   sequence number); +inf costs and (with both group arrays) sequences of the phrase's group are not admissible.  cand_dev
 *   [n_phrases, m] int32 padded with -1, coarse_dev [n_phrases, m] fp32 padded with +inf: bitwise independent of the cuts, of the
 *   packing and chunking of phrases and of what the workspace held.
 * sylber_dtw_rerank: q_dev [n_blocks * 128, D] the packed fp32 phrase rows, q_norm_dev as above (L2; may be null under IP),
 *   phrase_row_dev / phrase_len_dev [n_phrases]: first packed row (sylber_dtw_plan's phrase_row_host) and length of each phrase;
 *   seq_offsets_dev [n_seq + 1].  For every candidate of cand_dev [n_phrases, m] (-1 = none) the cost, start and end of
 *   sylber_dtw_search for that (phrase, sequence) pair, bit for bit; pairs of cost +inf dropped; ordered by (cost, sequence), the
 *   best k (1 <= k <= m) reported and padded as sylber_dtw_search reports them.
 * workspace_dev of either: sylber_dtw16_workspace_bytes(n_phrases, m, cuts) bytes (-1 on a bad argument); the re-rank may reuse
 *   the scan's on the same stream. */
int64_t sylber_dtw16_workspace_bytes(int32_t n_phrases, int32_t m, int32_t cuts);
int sylber_dtw16_scan(const void* q16_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                      const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const void* db16_dev, int32_t N, int32_t D,
                      const float* db_norm_dev, const float* q_norm_dev, int32_t metric, int32_t storage, int32_t m,
                      const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                      const int32_t* seq_group_dev, int32_t* cand_dev, float* coarse_dev, void* workspace_dev, void* stream);
int sylber_dtw_rerank(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                      const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev,
                      int32_t metric, const int32_t* cand_dev, int32_t m, const int32_t* seq_offsets_dev, int32_t n_seq, int32_t k,
                      float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream);

/* Every occurrence of a phrase (sylber_amd/search.py: SyllableIndex.search_occurrences / search_occurrences_refined; restated in
 * tests/occ_ref.py): every non-overlapping occurrence of a phrase in a sequence instead of the sequence's best one.  Local costs d,
 * the recurrence, the predecessor order on ties, start[i][j] and the NaN -> +inf rule are sylber_dtw_search's, word for word.  For
 * one phrase (m rows) and one sequence (columns 0 .. L - 1) let E[j] = A[m-1][j] and st[j] = start[m-1][j].
 *   1. Families.  Only columns with E[j] < +inf count (the start of an infinite cell carries no meaning and is not looked at).
 *      Columns with equal st[j] form a family: start = st[j], cost = min E[j], end = the smallest such j.  Over the finite columns
 *      st[j] does not decrease as j grows (two paths that would cross share a cell, and a cell has one predecessor chain), so a
 *      family is a run of neighbouring finite columns and families arrive in ascending start and ascending end.
 *   2. One left-to-right pass keeps non-overlapping families.  The first family becomes pending.  For each later family F: if
 *      F.start <= pending.end (the spans share a row) the cheaper of the two stays pending, the pending one on equal cost;
 *      otherwise the pending family is emitted and F becomes pending.  At the sequence end the pending family is emitted.  Emitted
 *      occurrences of one sequence are pairwise disjoint, and each is a real warping path with the cost, start and end the
 *      recurrence gives it.
 *   3. Per phrase the k best emitted occurrences over all admissible sequences (the group arrays mean what they mean for
 *      sylber_dtw_search), ordered strictly by (cost, first row of the span) ascending -- row ids ascend with sequence numbers, so
 *      this refines sylber_dtw_search's (cost, sequence) -- and padded with (+inf, -1, (-1, -1)).
 *   So: the best occurrence of a sequence under (cost, start) is bit for bit sylber_dtw_search's (cost, span) of that pair; for
 *   one-row phrases every finite row is an occurrence (sylber_knn_search with ids = span starts); nothing depends on the cuts, the
 *   packing or chunking of phrases or what the workspace held.
 *   The pass is NOT global greedy suppression by cost: of a chain A - B - C with A and C disjoint, both overlapping B, and costs
 *   A > B > C it emits only C (B beats A, C beats B), where greedy suppression would keep C and A.  The one-pass rule is what runs
 *   inside the scan with constant state per lane.
 * sylber_dtw_occurrences: sylber_dtw_search's arguments, sylber_dtw_plan's packing and cuts, a workspace of
 *   sylber_dtw_workspace_bytes(n_blocks, n_phrases, k, cuts) bytes.  cost_dev [n_phrases, k] fp32, seq_dev [n_phrases, k] int64
 *   (the sequence of each occurrence), span_dev [n_phrases, k, 2] int64 (first row, one past the last row).
 * sylber_dtw_rerank_occurrences: sylber_dtw_rerank's arguments; for the candidate sequences of cand_dev [n_phrases, m] (-1 = none;
 *   the candidates of one phrase must be distinct, as sylber_dtw16_scan's are) the occurrences of sylber_dtw_occurrences restricted
 *   to those sequences, bit for bit, the best k (1 <= k <= 128, not bounded by m) per phrase.  It excludes nothing: the stage that
 *   chose the candidates did.  workspace_dev: sylber_dtw_occ_workspace_bytes(n_phrases, m, k) bytes (-1 on a bad argument),
 *   O(P m k): m lists of k per phrase and their merge rounds.
 * Both refuse n_phrases x lists x k beyond 2^30 entries (status 1, sylber_last_error): use smaller phrase chunks. */
int sylber_dtw_occurrences(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                           const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N,
                           int32_t D, const float* db_norm_dev, int32_t metric, int32_t k, const int32_t* seq_id_dev,
                           const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev,
                           float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream);
int64_t sylber_dtw_occ_workspace_bytes(int32_t n_phrases, int32_t m, int32_t k);
int sylber_dtw_rerank_occurrences(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                  const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D,
                                  const float* db_norm_dev, int32_t metric, const int32_t* cand_dev, int32_t m,
                                  const int32_t* seq_offsets_dev, int32_t n_seq, int32_t k, float* cost_dev, int64_t* seq_dev,
                                  int64_t* span_dev, void* workspace_dev, void* stream);

/* Embedding repeats (sylber_amd/search.py: SyllableIndex.search_repeats / find_repeats; csrc/dtw_local.hip; restated in
 * tests/repeats_ref.py): LOCAL alignment of a probe (m rows, 1 <= m <= 64, prepared exactly as a phrase of sylber_dtw_search) against
 * every sequence (at most 65 536 rows) -- which part of the probe is said where in the sequence; both ends of both spans are free.
 * The local cost d[i][j] is sylber_dtw_search's, word for word (s0 = fmaf(-2, q_i . x_j, c_j) from the same contraction with the same
 * bits, then the L2 / IP forms; a NaN d counts as +inf).  radius > 0 and gap >= 0 are finite fp32.  Everything below is fp32 with one
 * rounding per operation, exactly as written:
 *   s  = radius - d[i][j]            (-inf where d = +inf)
 *   sg = s - gap
 *   H[i][-1] = H[-1][j] = 0
 *   c_diag = H[i-1][j-1] + s     start: start[i-1][j-1] if H[i-1][j-1] > 0 else (i, j)
 *   c_up   = H[i-1][j]   + sg    start: start[i-1][j]
 *   c_left = H[i][j-1]   + sg    start: start[i][j-1]
 *   v = the first largest of (c_diag, c_up, c_left) in that order; H[i][j] = v if v > 0 else 0
 * Every step lands on a cell and earns that cell's s; a non-diagonal step (one syllable said as two, a syllable without a partner)
 * also pays gap.  gap = 0 is a local DTW with free warping, a large gap is Smith-Waterman without gaps.
 * Result of (probe, sequence): the best cell -- the largest H, then the smallest i, then the smallest j; score = H[i][j];
 * (si, sj) = start[i][j]; the probe span is [si, i + 1), the sequence span [sj, j + 1) as row ids.  No positive cell: no result.
 *   Facts (held in tests/test_repeats_ref.py).  A predecessor with H = 0 is never strictly better through c_up / c_left than c_diag
 *   (gap >= 0), so start is only ever read from a positive cell, both spans are non-empty and the first cell of a path has s > 0.
 *   fp32 addition is monotone, so H[i][j] is the maximum over paths of the path's left-to-right fp32 sum: restricting the probe to a
 *   sub-range of its rows never raises a score, and a path that lies inside the sub-range keeps its bits.
 * Per probe an admissible result has score >= min_score (finite, > 0), a sequence numbered > after_seq[p] (where given) and, with
 * both group arrays, a sequence whose group differs from the probe's.  The k best admissible sequences are ordered strictly by
 * (score descending, sequence ascending); padding is score 0, sequence -1, spans -1.  Nothing depends on the cuts, the packing or
 * chunking of probes or what the workspace held.
 * sylber_dtw_local: sylber_dtw_search's arguments with sylber_dtw_plan's packing and cuts; radius, gap, min_score as above;
 *   after_seq_dev [n_phrases] int32 or null.  score_dev [n_phrases, k] fp32, seq_dev [n_phrases, k] int64, span_dev
 *   [n_phrases, k, 2, 2] int64: span[p][r][0] = (si, i + 1) positions inside the probe, span[p][r][1] = (sj, j + 1) row ids.
 *   workspace_dev: sylber_dtw_workspace_bytes(n_blocks, n_phrases, k, cuts) bytes (the lists keep their 16-byte entries:
 *   (-score, sequence, (sj row, (j - sj) | i << 16 | si << 22))).  Every argument is checked on the host before any device call:
 *   status 1 with sylber_last_error set. */
int sylber_dtw_local(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                     const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N, int32_t D,
                     const float* db_norm_dev, int32_t metric, int32_t k, float radius, float gap, float min_score,
                     const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                     const int32_t* seq_group_dev, const int32_t* after_seq_dev, float* score_dev, int64_t* seq_dev, int64_t* span_dev,
                     void* workspace_dev, void* stream);

/* Unit search (sylber_amd/units.py: UnitIndex.search_phrases / search_occurrences; csrc/unit_search.hip; restated in
 * tests/unit_search_ref.py): where is a phrase of syllable UNIT IDS said, by semi-global edit distance (Sellers' approximate
 * string matching).  The corpus holds tokens only: no embedding is needed.  A unit is a row of W non-negative int32 ids
 * (1 <= W <= 8: 1 for k-means units, 2 for residual units, Qa + Qp for the learned quantizer).  For phrase unit p_i
 * (i = 0 .. m-1, 1 <= m <= 64) and sequence unit t_j (j = 0 .. L-1, 1 <= L <= 65536), all in int32:
 *     sub(i, j) = number of columns c with p_i[c] != t_j[c]   (0 .. W);   an insertion or a deletion costs W
 *     E[-1][j] = 0,            start[-1][j] = j + 1           (j = -1 .. L-1: the phrase may begin anywhere)
 *     E[i][-1] = (i + 1) W,    start[i][-1] = 0
 *     E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W)
 *                on equal values the predecessor is taken in that order (diagonal, then (i-1, j), then (i, j-1)), the order of
 *                sylber_dtw_search; start[i][j] = start of the predecessor taken
 *   A column j of the last row is admissible when E[m-1][j] <= thr, thr = min(thr_host[p], m W - 1).  An admissible column has a
 *   path with a diagonal step, so start <= j and its span is never empty.
 * sylber_unit_search: per (phrase, sequence) cost = min E[m-1][j] over the admissible columns, end = the smallest such j, start =
 *   start[m-1][end]; a sequence without an admissible column is not returned.  Per phrase the k best sequences by
 *   (cost, sequence) ascending.
 * sylber_unit_occurrences: the three steps of "Every occurrence of a phrase" above, word for word, with "admissible" in place of
 *   "finite": families of admissible columns with equal start (cost = their minimum, end = the smallest such j; starts do not
 *   decrease with j, so they arrive in order), the one-pass left-to-right rule (on overlap the cheaper family stays pending, the
 *   pending one on equal cost), per phrase the k best emitted occurrences by (cost, first row).
 * Both: phrase_units_dev [R, W] holds the phrases' units, phrase p in rows phrase_row_host[p] .. + phrase_len_host[p]; units_dev
 *   [N, W] the corpus; seq_offsets_host [n_seq + 1] ascends from 0 to N without an empty sequence; seq_id_dev [N] is the sequence of
 *   every row; phrase_group_host [n_phrases] and seq_group_dev [n_seq] go together (both null: nothing excluded) and exclude the
 *   sequences of the phrase's own group; splits: 0 = automatic, else the cuts of the corpus asked for (cuts fall on sequence
 *   starts).  Out: cost_dev [n_phrases, k] int32, seq_dev [n_phrases, k] int64, span_dev [n_phrases, k, 2] int64 (first row, one
 *   past the last row), padded with (2^31 - 1, -1, (-1, -1)).  Costs are small integers: every result is exact and unique, and
 *   nothing depends on splits, the chunking of phrases or what the workspace held.  The host arrays are read before the call
 *   returns; everything else is enqueued on `stream`.  workspace_dev: sylber_unit_workspace_bytes of the same phrase lengths,
 *   offsets, k and splits (-1 on a bad argument).
 *   Every argument is checked on the host before any device call: a null pointer, W outside 1..8, k outside 1..128, a phrase of
 *   fewer than 1 or more than 64 units or outside its R rows, a sequence over 65536 rows, offsets that do not ascend from 0 to N,
 *   thr < 0, one group array without the other, n_phrases x cuts x k beyond 2^30 return status 1 with sylber_last_error set. */
int64_t sylber_unit_workspace_bytes(const int32_t* phrase_len_host, int32_t n_phrases, const int32_t* seq_offsets_host, int32_t n_seq,
                                    int32_t k, int32_t splits);
int sylber_unit_search(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_host,
                       const int32_t* phrase_len_host, const int32_t* thr_host, int32_t n_phrases, const int32_t* units_dev, int32_t N,
                       const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* seq_id_dev, const int32_t* phrase_group_host,
                       const int32_t* seq_group_dev, int32_t splits, int32_t k, int32_t* cost_dev, int64_t* seq_dev, int64_t* span_dev,
                       void* workspace_dev, void* stream);
int sylber_unit_occurrences(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_host,
                            const int32_t* phrase_len_host, const int32_t* thr_host, int32_t n_phrases, const int32_t* units_dev, int32_t N,
                            const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* seq_id_dev, const int32_t* phrase_group_host,
                            const int32_t* seq_group_dev, int32_t splits, int32_t k, int32_t* cost_dev, int64_t* seq_dev,
                            int64_t* span_dev, void* workspace_dev, void* stream);

/* Edit scripts (sylber_amd/units.py: UnitIndex.align_phrases; csrc/unit_align.hip; restated in tests/unit_align_ref.py): HOW a
 * phrase of units matches a window of rows -- which stored row each phrase unit is paired with and what was substituted, deleted
 * and inserted -- where the unit searches above report only where.  For one pair (phrase of m units, window [a, b) of row ids,
 * L = b - a columns):
 *   Window DP.  sub(i, j), the recurrence, the predecessor order on ties (diagonal, then (i-1, j), then (i, j-1): the first
 *   smallest) and the int32 arithmetic are unit search's.  The window is taken as ONE sequence whose column 0 is row a, even if it
 *   crosses a sequence boundary of the index.  The boundary column is E[i][-1] = (i + 1) W.  The boundary row depends on free_start:
 *     free_start = 1: E[-1][j] = 0: the phrase may begin anywhere in the window; this is the searches' DP.
 *     free_start = 0 (global): E[-1][j] = (j + 1) W with predecessor "left": the whole window is consumed, so cost is the weighted
 *       Levenshtein distance of phrase and window.
 *   The end is forced: the path ends in cell (m-1, L-1).
 *   Path.  The chain of predecessors taken from (m-1, L-1) back to the boundary.  Under free_start = 1 it stops at row -1 in some
 *   column j (the first row of the path is a + j + 1) or at column -1 in some row i (phrase units 0 .. i are deletions, the first
 *   row is a).  Under free_start = 0 it runs on along row -1 to the corner: those steps are leading insertions and the first row is a.
 *   Outputs.  cols[i] = the row id that phrase unit i is paired with by a diagonal step, -1 if unit i is deleted or i >= m;
 *   subs[i] = sub(i, j) of that pairing (0 .. W), W for a deleted unit, -1 for i >= m; ops = (equal, substituted, deleted,
 *   inserted): diagonal steps with sub = 0, diagonal steps with sub > 0, phrase units without a row, rows of the path without a
 *   phrase unit; cost = E[m-1][L-1].  By construction equal + substituted + deleted = m, the first row of the path =
 *   b - (equal + substituted + inserted), cost = sum(subs[:m]) + W * inserted, and the sum of ops is the number of edit operations,
 *   the divisor of a length-normalised cost.  Every legal window has a finite cost.
 *   The theorem.  If [a, b) is a span that sylber_unit_search or sylber_unit_occurrences returned for that phrase on those rows,
 *   then in either mode (1) the path's first row is a, (2) cost is the reported cost, (3) the path is the scan's own path.  Why, as
 *   for "Warping paths" below and simpler in int32: a window cell is a minimum over fewer paths, so it is never below the full
 *   DP's cell; the window boundary (i + 1) W is what a run of deletions from row -1 costs in the full DP; on the scan's path the
 *   two DPs are equal; a predecessor that lost in the full DP was strictly larger there and still is, so the same one wins.
 *   tests/test_unit_align_ref.py holds it on more than 20 000 returned spans.  So no scan had to keep its path.
 *   Any other window is legal and gets what the definition gives; under free_start = 1 its path may begin inside the window.
 *   Nothing returned depends on how pairs are chunked or on what the workspace held.
 * sylber_unit_align: phrase_units_dev [R, W] and units_dev [N, W] as for sylber_unit_search; phrase_row_dev, phrase_len_dev
 *   [n_phrases] int32 on the DEVICE: phrase p is rows phrase_row[p] .. + phrase_len[p].  pair_phrase_dev [n_pairs] int32: the
 *   phrase of each pair; pair_window_dev [n_pairs, 2] int32: (a, b), (-1, -1) = none; max_cols: no window is longer (1 .. 65 536);
 *   max_rows: the pitch Mx of cols_dev and subs_dev, at least the longest phrase (1 .. 64); free_start: 0 or 1.  Out: cols_dev,
 *   subs_dev [n_pairs, max_rows] int32, ops_dev [n_pairs, 4] int32, cost_dev [n_pairs] int32; start_dev [n_pairs] int32, may be
 *   null: the first row as the forward walk itself tracked it through the cells, as the scans track theirs (free_start = 0: a) --
 *   always b - (equal + substituted + inserted); a check of the codes, not a result.  workspace_dev:
 *   sylber_unit_align_workspace_bytes(n_pairs, max_cols) = 16 B per column of max_cols + 63 steps, rounded up to chunks of 32, per
 *   pair (-1 on a bad argument): 2 bits per cell for the predecessor taken.
 *   A null pointer other than start_dev, W outside 1..8, R, N, n_phrases or n_pairs below 1, max_cols outside 1..65 536, max_rows
 *   outside 1..64 and free_start outside {0, 1} return 1 with sylber_last_error before any device call.  The windows and the
 *   phrase tables are device data that the entry cannot see: the caller validates them (align_phrases does, with one reduction,
 *   before any launch), and a pair whose phrase number lies outside [0, n_phrases), whose phrase has fewer than 1 or more than
 *   min(64, max_rows) units or rows outside R, or whose window lies outside [0, N], is empty or is longer than max_cols is padding
 *   on output -- cols and subs -1, ops 0, cost 2^31 - 1, start -1 -- having read and written nothing but that. */
int64_t sylber_unit_align_workspace_bytes(int32_t n_pairs, int32_t max_cols);
int sylber_unit_align(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_dev, const int32_t* phrase_len_dev,
                      int32_t n_phrases, const int32_t* units_dev, int32_t N, const int32_t* pair_phrase_dev, const int32_t* pair_window_dev,
                      int32_t n_pairs, int32_t max_cols, int32_t max_rows, int32_t free_start, int32_t* cols_dev, int32_t* subs_dev,
                      int32_t* ops_dev, int32_t* cost_dev, int32_t* start_dev /* nullable */, void* workspace_dev, void* stream);

/* Unit strings (sylber_amd/units.py: align_unit_strings / unit_error_rate; csrc/unit_strings.hip; restated in
 * tests/unit_strings_ref.py): how far two tokenisations of the same audio are from each other -- the global alignment of WHOLE
 * unit strings, without the 64-unit limit of "Edit scripts", many pairs per call.  A pair is a reference string r of m units and a
 * hypothesis string h of L units, 0 <= m, L <= 65 536; a unit is a row of W ids, 1 <= W <= 8, ids in 0 .. 2^31 - 1;
 * sub(i, j) = the number of columns in which r[i] and h[j] differ.  The DP, all int32:
 *     E[i][-1] = (i + 1) W        E[-1][j] = (j + 1) W  (predecessor "left")        E[-1][-1] = 0
 *     E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W)   the first smallest in that order
 *   The path is the chain of predecessors from (m-1, L-1) to the corner.
 *   Outputs per pair.  cost = E[m-1][L-1].  ops = (equal, substituted, deleted, inserted): diagonal steps with sub = 0, diagonal
 *   steps with sub > 0, reference units without a partner, hypothesis units without one.  With pairing, cols[i] = the position
 *   INSIDE h (0-based) that reference unit i met on a diagonal step, -1 if the unit is deleted, and subs[i] = that sub, W for a
 *   deleted unit.
 *   Empty sides.  m = 0: cost L W, ops (0, 0, 0, L).  L = 0: cost m W, ops (0, 0, m, 0), every cols -1 and every subs W.
 *   Identities.  equal + substituted + deleted = m; equal + substituted + inserted = L; cost = sum(subs) + W * inserted.
 *   For 1 <= m <= 64 and L >= 1 this is sylber_unit_align with free_start = 0 on the window [0, L) of h: cost, ops, cols and subs,
 *   bit for bit.  Only cost is symmetric under exchanging r and h; the counts are not, since ties resolve differently.
 *   Counts without a path.  A cell carries (cost, d, sb): d = the diagonal steps on the path that the chosen predecessor tracked,
 *   sb = those of them with sub > 0, both 0 on row -1 and column -1; then equal = d - sb, substituted = sb, deleted = m - d,
 *   inserted = L - d.  ops_dev is written from these counters in both modes; with pairing the walk back over the predecessor codes
 *   counts its own four and writes them to ops_walk_dev where that is not null -- always equal to ops_dev; a check of the codes,
 *   not a result.
 *   Nothing returned depends on what the workspace held, on which pairs share a call or on their order: a pair touches only its
 *   own slice of the workspace and its own outputs.
 * sylber_unit_strings_align: ref_units_dev [ref_offsets_host[n_pairs], W] and hyp_units_dev [hyp_offsets_host[n_pairs], W] int32 on
 *   the device; pair p is reference rows ref_offsets_host[p] .. ref_offsets_host[p + 1] against hypothesis rows
 *   hyp_offsets_host[p] .. hyp_offsets_host[p + 1].  The offsets [n_pairs + 1] ascend from 0 and may repeat (empty strings); they
 *   are read before the call returns, everything else is enqueued on `stream`.  pairing: 0 = counts only, 1 = cols_dev and
 *   subs_dev [ref_offsets_host[n_pairs]] int32 too (required iff pairing).  ops_dev [n_pairs, 4], cost_dev [n_pairs] int32;
 *   ops_walk_dev [n_pairs, 4] may be null and is written with pairing only.
 *   workspace_dev: sylber_unit_strings_workspace_bytes of the same offsets and pairing, host arithmetic on the lengths (-1 on a bad
 *   argument), every term rounded up to 256 B:
 *       48 B per pair of table
 *     + 24 L per pair with m > 64 and L > 0: two rows of (cost, d, sb) between strips of 64 reference rows, at most 1.5 MiB
 *     + with pairing, ceil(m / 64) * ceil((L + 63) / 32) * 512 B per pair with m, L > 0: 2 bits per cell, about m L / 4.
 *   A null pointer other than ops_walk_dev (and cols_dev, subs_dev without pairing), W outside 1..8, n_pairs < 1, pairing outside
 *   {0, 1}, offsets that do not start at 0 or that descend, and a string of more than 65 536 units return 1 with
 *   sylber_last_error before any device call. */
int64_t sylber_unit_strings_workspace_bytes(const int32_t* ref_offsets_host, const int32_t* hyp_offsets_host, int32_t n_pairs,
                                            int32_t pairing);
int sylber_unit_strings_align(const int32_t* ref_units_dev, const int32_t* ref_offsets_host, const int32_t* hyp_units_dev,
                              const int32_t* hyp_offsets_host, int32_t W, int32_t n_pairs, int32_t pairing, int32_t* cols_dev,
                              int32_t* subs_dev, int32_t* ops_dev, int32_t* cost_dev, int32_t* ops_walk_dev /* nullable */,
                              void* workspace_dev, void* stream);

/* Unit repeats (sylber_amd/units.py: local_align_unit_strings / UnitIndex.find_repeats; csrc/unit_repeats.hip; restated in
 * tests/unit_repeats_ref.py): what is said in BOTH of two recordings, found without a query -- the local alignment
 * (Smith-Waterman) of two unit strings, the best-scoring pair of sub-spans, many pairs per call.  A pair is a string x of m units
 * and a string y of L units, 0 <= m, L <= 65 536; a unit is a row of W ids, 1 <= W <= 8, ids in 0 .. 2^31 - 1; sub(i, j) = the
 * number of columns in which x[i] and y[j] differ.  Parameters: 1 <= match <= 64 (2), 0 <= mismatch <= 64 (3), 1 <= gap <= 64
 * (4).  The DP, all int32 (scores stay below 64 * 8 * 65 536):
 *     s(i, j)  = match * (W - sub(i, j)) - mismatch * sub(i, j)
 *     H[i][-1] = H[-1][j] = 0
 *     c_diag   = H[i-1][j-1] + s(i, j)     start: start[i-1][j-1] if H[i-1][j-1] > 0, else (i, j)
 *     c_up     = H[i-1][j]   - gap * W     start: start[i-1][j]
 *     c_left   = H[i][j-1]   - gap * W     start: start[i][j-1]
 *     v        = the first largest of (c_diag, c_up, c_left), in that order
 *     H[i][j]  = v if v > 0 else 0         start[i][j] = that candidate's start (unused where H = 0)
 *   x is the rows and y the columns: the ties depend on it, so the two are not exchanged.
 *   Outputs per pair: its best cell (i, j) = the largest H[i][j], on equal values the smallest i, then the smallest j.
 *   score = H[i][j]; with (si, sj) = start[i][j] the spans are x[si : i + 1] and y[sj : j + 1], written as
 *   span = (a0, a1, b0, b1) = (si, i + 1, sj, j + 1), positions INSIDE the two windows.  A pair without a positive cell -- an empty
 *   side included -- has score 0 and span (-1, -1, -1, -1).
 *   Consequences.  Both spans are non-empty: the first and the last step of the path are diagonal steps with s > 0.  When
 *   gap = mismatch + match / 2 with match even, score = match * W * ((a1 - a0) + (b1 - b0)) / 2 - (match + mismatch) * cost, cost =
 *   the weighted Levenshtein distance of the two spans ("Unit strings"); under the defaults score = W * (len_x + len_y) - 5 cost.
 *   Nothing returned depends on what the workspace held, on which pairs share a call or on their order: a pair touches only its
 *   own slice of the workspace and its own outputs.
 * sylber_unit_local_align: x_units_dev [x_rows, W] and y_units_dev [y_rows, W] int32 on the device; x_win_host and y_win_host
 *   [n_pairs, 2] int32 = (first row, number of rows) of each pair's window into its buffer.  The two buffers may be the same
 *   buffer, windows may overlap and may repeat: that is how one corpus is aligned against itself.  The windows are read before the
 *   call returns, everything else is enqueued on `stream`.  score_dev [n_pairs], span_dev [n_pairs, 4] int32.
 *   workspace_dev: sylber_unit_local_workspace_bytes of the same windows, host arithmetic on the lengths (-1 on a bad argument),
 *   every term rounded up to 256 B:
 *       40 B per pair of table
 *     + 24 L per pair with m > 64 and L > 0: two rows of (H, si, sj), 12 B per column, between strips of 64 rows of x, at most
 *       1.5 MiB.
 *   A null pointer, W outside 1..8, n_pairs < 1, match, mismatch or gap outside its range, a window with a negative length or of
 *   more than 65 536 rows and a window outside its buffer return 1 with sylber_last_error before any device call. */
int64_t sylber_unit_local_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs);
int sylber_unit_local_align(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                            const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t match, int32_t mismatch,
                            int32_t gap, int32_t* score_dev /* [n_pairs] */, int32_t* span_dev /* [n_pairs, 4] */,
                            void* workspace_dev, void* stream);

/* Unit repeats, every one (sylber_amd/units.py: local_align_unit_strings_all / UnitIndex.find_repeats with per_pair or within;
 * csrc/unit_repeats_all.hip; restated in tests/unit_repeats_all_ref.py): EVERY phrase two unit strings share, and the phrases one
 * string says more than once -- up to n_best repeats per pair, found round by round without a traceback.  A pair is x (m units)
 * and y (L units); widths, the id range, match / mismatch / gap and the limit of 65 536 units are those of "Unit repeats".  Three
 * more parameters: n_best = R, 1 <= R <= 32; min_score >= 1; per pair sep >= 0.
 *   The rounds r = 0 .. R - 1 run in order.  Round r computes the recurrence of "Unit repeats" word for word with one change: a
 *   BLOCKED cell has H = 0, carries no start and is never the best cell.  Cell (i, j) is blocked in round r when
 *     * sep > 0 and j - i < sep: the band on and below the diagonal, for x and y the same string (sep = 1 leaves only j > i, so
 *       every repeat is found once and no unit is matched with itself), or
 *     * a0 <= i < a1 and b0 <= j < b1 for the span (a0, a1, b0, b1) that an earlier round of this pair returned: the rectangle
 *       of an earlier repeat.
 *   The result of round r is the best unblocked cell in the order of "Unit repeats": the largest H, then the smallest i, then the
 *   smallest j; score = H[i][j], span = (si, i + 1, sj, j + 1).  If a round's score is below min_score, that round and every
 *   later one return score 0 and span (-1, -1, -1, -1), and the pair does no further DP work; so does every round of a pair with
 *   an empty side.
 *   Why rectangles.  The kernel keeps no traceback and a rectangle needs none: every cell of a round's path lies inside the
 *   round's rectangle, and a path never contains a blocked cell -- a diagonal step out of H = 0 starts anew and an up or left
 *   step out of it is negative.  The rectangle also removes the shadow alignments that hug a found path.
 *   Consequences (tests/test_unit_repeats_all_ref.py).  Round 0 with sep = 0 and min_score = 1 is "Unit repeats" bit for bit.
 *   Blocking only lowers H, so scores never increase from round to round.  A phrase said once in x and twice in y comes back as
 *   two rounds with the same x span; three occurrences p1 < p2 < p3 inside one string with sep = 1 come back as the three repeats
 *   (p1, p2), (p1, p3), (p2, p3).  Rectangles of different rounds may intersect as rectangles; no cell of a round's path lies in
 *   an earlier rectangle.  With sep > 0 the two spans of a repeat may overlap, as in tandem repetition: [1, 2, 3] * 10 against
 *   itself with sep = 1 gives one repeat, x[0:27] against y[3:30].  a1 <= b0 is the caller's filter; the DP does not enforce it.
 *   Nothing returned depends on what the workspace held, on which pairs share a call or on their order.
 * sylber_unit_local_align_all: buffers and windows as for sylber_unit_local_align.  sep_host [n_pairs] int32 may be null: all 0.
 *   The windows and sep_host are read before the call returns, everything else is enqueued on `stream`: ONE launch runs all the
 *   rounds of every pair, one 64-thread workgroup per pair, the pair's rectangles in LDS.  score_dev [n_pairs, n_best],
 *   span_dev [n_pairs, n_best, 4] int32.
 *   workspace_dev: sylber_unit_local_all_workspace_bytes of the same windows, host arithmetic on the lengths (-1 on a bad
 *   argument), every term rounded up to 256 B:
 *       48 B per pair of table
 *     + 24 L per pair with m > 64 and L > 0: the two rows between strips, as for sylber_unit_local_align; every round uses them
 *       again.
 *   What sylber_unit_local_align refuses, n_best outside 1..32, min_score < 1 and a negative sep return 1 with sylber_last_error
 *   before any device call. */
int64_t sylber_unit_local_all_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs);
int sylber_unit_local_align_all(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                                const int32_t* x_win_host, const int32_t* y_win_host, const int32_t* sep_host /* nullable: all 0 */,
                                int32_t n_pairs, int32_t match, int32_t mismatch, int32_t gap, int32_t n_best, int32_t min_score,
                                int32_t* score_dev /* [n_pairs, n_best] */, int32_t* span_dev /* [n_pairs, n_best, 4] */,
                                void* workspace_dev, void* stream);

/* Warping paths(sylber_amd/search.py: SyllableIndex.align_phrases; restated in tests/align_ref.py): HOW a phrase matches a
 * window of rows -- which stored rows each phrase row is warped onto -- where the searches above report only where.  For one pair
 * (phrase of m rows, window [a, b) of row ids, W = b - a):
 *   Window DP.  The local costs d[i][j] are sylber_dtw_search's, bit for bit (the ascending fmaf chain from 0 over D of
 *   sylber_dtw_rerank, then the same d).  The window is taken as ONE sequence whose first column is a: a free start (A[0][j] =
 *   d[0][j] for every column of the window) and a forced end: the path ends in cell (m-1, b-1).  The recurrence and the predecessor
 *   order on ties are sylber_dtw_search's, unchanged: diagonal, then (i-1, j), then (i, j-1).
 *   Path and outputs.  The path is the chain of predecessors taken from (m-1, b-1) back to the row-0 cell it reaches.  cost =
 *   A[m-1][b-1]; steps = the number of cells on the path; rows[i] = (first row id, one past the last row id) of the run of columns
 *   the path visits in phrase row i.  A monotone path visits one contiguous run per row and lo[i+1] is hi[i] or hi[i] + 1, so the
 *   runs ARE the path.  If A[m-1][b-1] is not below +inf the pair is padding on output: rows (-1, -1), steps 0, cost +inf.
 *   The theorem.  If [a, b) is a span that a phrase search of this library returned for that phrase under the same metric and rows,
 *   then (1) the path starts in column a, (2) cost has the bits of the reported cost, (3) the path is the full scan's own path.
 *   Why: every window cell's A is at least the full DP's (it is a minimum over fewer paths and fp32 + is monotone), and on the
 *   optimal path the two are equal, so at every cell of that path the first smallest predecessor is the same one.
 *   tests/test_align_ref.py holds it on random, tied and +inf-holed matrices.  So no scan had to keep its path.
 *   Any other window is legal and gets what the definition gives; its path may start inside the window.  steps is the divisor of
 *   a length-normalised DTW cost: cost / steps.
 *   Nothing returned depends on how pairs are chunked or on what the workspace held.
 * sylber_dtw_align: q_dev, n_blocks, q_norm_dev, phrase_row_dev, phrase_len_dev, n_phrases, db_dev, N, D, db_norm_dev, metric as
 *   for sylber_dtw_rerank.  pair_phrase_dev [n_pairs] int32: the phrase of each pair; pair_window_dev [n_pairs, 2] int32: (a, b),
 *   (-1, -1) = none; max_cols: no window is longer (1 .. 65 536); max_rows: the row pitch Mx of rows_dev, at least the longest
 *   phrase (1 .. 64).  rows_dev [n_pairs, max_rows, 2] int32, (-1, -1) for i >= m and for padding; steps_dev [n_pairs] int32;
 *   cost_dev [n_pairs] fp32; start_dev [n_pairs] int32, may be null: the start row that the walk itself tracked for (m-1, b-1),
 *   as sylber_dtw_rerank tracks it (-1 for padding) -- always rows_dev[pair][0][0]; a check of the codes, not a result.  workspace_dev: sylber_dtw_align_workspace_bytes(n_pairs, max_cols) = 16 B x (max_cols + 63) per pair
 *   (-1 on a bad argument): 2 bits per cell for the predecessor taken.  Bad arguments and max_cols > 65 536 return 1 with
 *   sylber_last_error before any device call.  The windows are device data that the entry cannot see: the caller validates them
 *   (align_phrases does, with one reduction, before any launch), and a pair whose window lies outside [0, N], is empty or is longer
 *   than max_cols reads and writes nothing beyond its outputs, which are padding. */
int64_t sylber_dtw_align_workspace_bytes(int32_t n_pairs, int32_t max_cols);
int sylber_dtw_align(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                     const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev,
                     int32_t metric, const int32_t* pair_phrase_dev, const int32_t* pair_window_dev, int32_t n_pairs, int32_t max_cols,
                     int32_t max_rows, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* start_dev, void* workspace_dev,
                     void* stream);

/* Embedding strings (sylber_amd/search.py: align_sequences / SyllableIndex.align_sequences; csrc/dtw_strings.hip; restated in
 * tests/dtw_strings_ref.py): how two WHOLE embedding sequences line up, row by row -- the global DTW of two recordings, without
 * the 64-row limit of a phrase, many pairs per call.  What "Unit strings" is to unit ids.  A pair is a sequence x of m rows and a
 * sequence y of L rows, 0 <= m, L <= 65 536; D is a multiple of 16 and at least 16.
 *   Local cost.  d[i][j] is sylber_dtw_search's, word for word, with x in the role of the phrase and y in the role of the
 *   database: dot = the ascending fmaf chain from 0 over D; s = fmaf(-2, dot, c_j); L2: c_j = ||y_j||^2 as sylber_knn_row_norms
 *   gives it and d = max(0, ||x_i||^2 + s); IP / cosine: both sides made unit rows by sylber_knn_unit_rows, c_j = 0 and
 *   d = max(0, 1 - (0 - s / 2)); a NaN d counts as +inf.  The kernel contracts on v_mfma_f32_32x32x2_f32 in sylber_dtw_search's
 *   k-pair order, which produces the bits of that chain.
 *   Global DTW, all additions in fp32, one per cell:
 *     A[0][0] = d[0][0]                                     n[0][0] = 1
 *     A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      terms outside the matrix are +inf
 *               the first smallest in that order (diagonal, up, left): the order of every DTW in this library
 *     n[i][j] = n[the predecessor taken] + 1
 *   Outputs per pair.  cost = A[m-1][L-1].  steps = n[m-1][L-1], the cells on the path: the divisor of the length-normalised
 *   distance cost / steps.  With path, rows[i] = (lo, hi) for every row i of x: the run of y positions the path visits in row i,
 *   0-based INSIDE y's window, hi exclusive, written at x's flat row rows_offset_host[pair] + i.  A monotone path visits one run
 *   per row; lo[0] = 0, hi[m-1] = L, and lo[i+1] is hi[i] - 1 or hi[i], so the runs ARE the path.
 *   Padding.  A pair whose cost is not below +inf is padding: cost +inf, steps 0, rows (-1, -1).  An empty side (m = 0 or L = 0)
 *   is padding too.
 *   Counts without a path.  A cell carries (A, n), the way "Unit strings" carries (cost, d, sb); the counts-only kernel writes no
 *   predecessor codes.  With path the walk back over the 2-bit codes counts its own cells and writes them to steps_walk_dev
 *   where that is not null -- always equal to steps_dev; a check of the codes, not a result.
 *   Nothing returned depends on what the workspace held, on which pairs share a call or on their order: a pair touches only its
 *   own slice of the workspace and its own outputs.
 *   The theorem.  Take a phrase x of at most 64 rows and a window [a, b) of rows.  If sylber_dtw_align's path for that pair
 *   starts in column a -- it does for every span that a phrase search returned -- then the global alignment of x against rows
 *   [a, b) has that cost, bit for bit, that steps, and those runs shifted by a.  Why: the window DP has a free start and a forced
 *   end, and the global DP minimises over a subset of its paths; fp32 + is monotone, so every global cell is at least the
 *   window cell, and on that path the two are equal; a predecessor that lost in the window DP was strictly larger there and
 *   still is; on an exact tie the global cell is not smaller, so the first-smallest order names the same winner whenever the
 *   winner lies on the common path.  Always: the global cost >= sylber_dtw_align's cost on the same window.
 *   tests/test_dtw_strings_ref.py holds both on random, tied and +inf-holed matrices.
 * sylber_dtw_strings_align: x_dev [x_rows, D] and y_dev [y_rows, D] fp32 on the device (unit rows under IP); x_norm_dev [x_rows]
 *   and y_norm_dev [y_rows] fp32: required under L2, may be null under IP; metric as for sylber_knn_search.  x_win_host and
 *   y_win_host [n_pairs, 2] int32 = (first row, number of rows) of each pair's window into its buffer.  The two buffers may be
 *   the same buffer, windows may overlap and may repeat.  The host arrays are read before the call returns, everything else is
 *   enqueued on `stream`.  path: 0 = cost and steps only, 1 = rows_dev [*, 2] int32 too, pair p at rows rows_offset_host[p] .. + m
 *   (rows_offset_host [n_pairs] int64 and rows_dev are required iff path).  steps_dev [n_pairs] int32, cost_dev [n_pairs] fp32;
 *   steps_walk_dev [n_pairs] may be null and is written with path only.
 *   workspace_dev: sylber_dtw_strings_workspace_bytes of the same windows and path, host arithmetic on the lengths (-1 on a bad
 *   argument), every term rounded up to 256 B:
 *       64 B per pair of table
 *     + 16 L per pair with m > 128 and L > 0: two alternating rows of (A, n), 8 B per column, between super-strips of 128 rows
 *       of x, at most 1 MiB
 *     + with path, ceil(m / 64) * ceil(L / 128) * 2048 B per pair with m, L > 0: 2 bits per cell, about m L / 4; one lane's 128
 *       cells of one tile are four 64-bit words.
 *   A null pointer other than the nullable ones (the norms under IP, steps_walk_dev, and rows_offset_host and rows_dev without
 *   path), D below 16 or no multiple of 16, an unknown metric, L2 without norms, n_pairs < 1, a window with a negative length or
 *   of more than 65 536 rows, a window outside its buffer, a negative rows_offset_host and path outside {0, 1} return 1 with
 *   sylber_last_error before any device call.  The windows are host data, so no stale table can reach the kernel; what it reads
 *   from the table is what this entry checked and wrote. */
int64_t sylber_dtw_strings_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path);
int sylber_dtw_strings_align(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                             const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host,
                             int32_t n_pairs, int32_t path, const int64_t* rows_offset_host /* [n_pairs], with path: x's flat row in rows_dev */,
                             int32_t* rows_dev /* [*, 2], with path */, int32_t* steps_dev, float* cost_dev,
                             int32_t* steps_walk_dev /* nullable */, void* workspace_dev, void* stream);
/* sylber_dtw_strings_align_split (csrc/dtw_strings_split.hip; the blocked recurrence restated in tests/dtw_strings_split_ref.py):
 *   sylber_dtw_strings_align with the work of ONE pair spread over many workgroups, for calls that bring few long pairs.  Every
 *   argument of sylber_dtw_strings_align means what it means there; block_rows and block_cols are the rows of x and the columns
 *   of y of a block, multiples of 128 up to 65 536, 0 = the library's choice (128 x 128, profiles/dtw_strings_split_bench.md).
 *   The block recurrence.  With BR = block_rows and BC = block_cols a pair has nbr = ceil(m / BR) bands of rows and
 *   nbc = ceil(L / BC) chunks of columns; block (b, c) holds the cells of rows [b BR, (b+1) BR) and columns [c BC, (c+1) BC)
 *   that lie in the matrix.  It computes them by the recurrence above from three inputs: the last row of block (b-1, c), the
 *   last column of block (b, c-1) and the corner cell (A, n)[b BR - 1][c BC - 1]; outside the matrix they are +inf.  Launch d
 *   runs every block with b + c = d of every pair of the call, one workgroup per block; a pair needs nbr + nbc - 1 launches and
 *   one more that writes its outputs, all on `stream`, and stream order is the only order between blocks: no workgroup waits
 *   for another.  Inside a block the cells are computed by the code of sylber_dtw_strings_align on the same global grid of
 *   128-column tiles and 64-row strips, the same operations in the same order, so cost, steps, rows and steps_walk are
 *   BIT FOR BIT sylber_dtw_strings_align's.  Nothing returned depends on the block sizes, on which pairs share a call, on
 *   their order or on what the workspace held: a block reads only cells that an earlier launch of the same call wrote.
 *   workspace_dev: sylber_dtw_strings_split_workspace_bytes of the same windows, path and block sizes, host arithmetic on the
 *   lengths (-1 on a bad argument), every term rounded up to 256 B:
 *       64 B per pair of table
 *     + per pair with m, L > 0:
 *         256 B: the last cell, from the block that holds it to the launch that writes the outputs
 *       + 16 L where nbr > 1: two boundary rows of (A, n), 8 B per column, alternating by the parity of b
 *       + 16 L where BR > 128 and m > 128: two rows between a block's own super-strips of 128 rows
 *       + 16 (m + nbr) where nbc > 1: two boundary columns of (A, n), 8 B per row, alternating by the parity of c, each band's
 *         cells led by one more: the corner of the block to the right, which travels with the column because the boundary
 *         row that holds it is rewritten in the launch that would read it
 *     + with path, the codes of sylber_dtw_strings_align, at the same places.
 *   Refused with status 1 and sylber_last_error before any device call: everything sylber_dtw_strings_align refuses, and a
 *   block_rows or block_cols that is negative, no multiple of 128 or above 65 536. */
int64_t sylber_dtw_strings_split_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path,
                                                 int32_t block_rows, int32_t block_cols);
int sylber_dtw_strings_align_split(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                                   const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host,
                                   int32_t n_pairs, int32_t path, const int64_t* rows_offset_host /* [n_pairs], with path */,
                                   int32_t* rows_dev /* [*, 2], with path */, int32_t* steps_dev, float* cost_dev,
                                   int32_t* steps_walk_dev /* nullable */, int32_t block_rows, int32_t block_cols, void* workspace_dev,
                                   void* stream);

/* Embedding strings, local(sylber_amd/search.py: local_align_sequences / SyllableIndex.local_align_sequences;
 * csrc/dtw_strings_local.hip; restated in tests/dtw_strings_local_ref.py): every repeat between two WHOLE embedding sequences --
 * the best sub-span of x against the best sub-span of y, up to n_best of them per pair, and with a band below the diagonal the
 * repeats inside ONE sequence.  "Embedding repeats" without the 64-row limit of a probe; what "Unit repeats, every one" is to
 * unit ids.  A pair is x of m rows and y of L rows, 0 <= m, L <= 65 536; D is a multiple of 16 and at least 16; d[i][j] is the
 * local cost of "Embedding strings" (sylber_dtw_search's, word for word; a NaN d counts as +inf).  radius > 0, gap >= 0 and
 * min_score > 0 are finite fp32; n_best = R, 1 <= R <= 32; per pair sep >= 0.
 *   Rounds r = 0 .. R-1 run in order; round r is the "Embedding repeats" recurrence unchanged, everything in fp32 with one rounding
 *   per operation:
 *     s = radius - d[i][j], sg = s - gap, H[i][-1] = H[-1][j] = 0
 *     c_diag = H[i-1][j-1] + s     start: start[i-1][j-1] if H[i-1][j-1] > 0 else (i, j)
 *     c_up   = H[i-1][j]   + sg    start: start[i-1][j]
 *     c_left = H[i][j-1]   + sg    start: start[i][j-1]
 *     v = the first largest of (c_diag, c_up, c_left) in that order; H[i][j] = v if v > 0 else 0
 *   Blocked cells, the one addition, from "Unit repeats, every one".  A blocked cell has H = 0, carries no start and is never the
 *   best cell.  (i, j) is blocked when sep > 0 and j - i < sep, or when a0 <= i < a1 and b0 <= j < b1 for the spans of an earlier
 *   round.  Rectangles of different rounds may intersect as rectangles; no cell of a round's path lies in an earlier rectangle.
 *   Result of a round: the best unblocked cell -- the largest H, then the smallest i, then the smallest j -- with score = H[i][j]
 *   and the spans [si, i + 1) of x and [sj, j + 1) of y, (si, sj) = start[i][j], positions INSIDE the two windows.  A round
 *   without a positive cell or with score < min_score ends the pair: it and every later round are score 0, spans -1.  An empty
 *   side gives padding only.  So: round 0 with sep = 0 is the "Embedding repeats" result of x as a probe of any length against y
 *   as one sequence, bit for bit, wherever its score reaches min_score; scores never increase from round to round.
 *   With sep > 0 the two spans of a repeat may overlap, as in tandem repetition; a1 <= b0 is the caller's filter.
 *   Nothing returned depends on what the workspace held, on which pairs share a call or on their order.
 *   Not built: blocking the cells of a path instead of its rectangle; one pair split across workgroups; the 16-bit and PQ forms.
 * sylber_dtw_strings_local: buffers, norms, metric and windows as for sylber_dtw_strings_align; x and y may be one buffer and the
 *   windows of a pair the same window (a sequence against itself, with sep >= 1).  sep_host [n_pairs] int32 may be null: all 0.
 *   The windows and sep_host are read before the call returns, everything else is enqueued on `stream`: ONE launch runs all the
 *   rounds of every pair, one 256-thread workgroup per pair; each round repeats the contraction, the costs are not kept.
 *   scores_dev fp32 [n_pairs, n_best]; spans_dev int32 [n_pairs, n_best, 4] = (a0, a1, b0, b1).
 *   workspace_dev: sylber_dtw_strings_local_workspace_bytes of the same windows, host arithmetic on the lengths (-1 on a bad
 *   argument), every term rounded up to 256 B; it does not grow with n_best:
 *       64 B per pair of table
 *     + 16 L per pair with m > 128 and L > 0: two alternating rows of (H, start), 8 B per column, between super-strips of 128 rows
 *       of x, at most 1 MiB; every round uses them again.
 *   What sylber_dtw_strings_align refuses of its buffers, norms, D, metric, n_pairs and windows, a radius, gap or min_score that
 *   is not finite or not > 0 (gap: >= 0), n_best outside 1..32 and a negative sep return 1 with sylber_last_error before any
 *   device call. */
int64_t sylber_dtw_strings_local_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs);
int sylber_dtw_strings_local(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                             const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host,
                             const int32_t* sep_host /* nullable: all 0 */, int32_t n_pairs, float radius, float gap, float min_score,
                             int32_t n_best, float* scores_dev /* [n_pairs, n_best] */, int32_t* spans_dev /* [n_pairs, n_best, 4] */,
                             void* workspace_dev, void* stream);

/* The exact DTW on a coded database (sylber_amd/pq.py: IVFPQSyllableIndex.search_phrases / search_occurrences / align_phrases with
 * rerank=False; restated in tests/ivfpq_phrase_ref.py): sylber_dtw_rerank and sylber_dtw_align with db_dev replaced by
 * product-quantization codes that may lie in another order than the row ids and may be codes of residuals to a list centroid.  No row is materialised: the kernels rebuild
 * each row inside the dot-product chain.  The coded database is one argument group, the same in every entry:
 *   code_dev [N, M] uint8 and bad_dev [N] uint8 (nullable; 1 = a masked row), both in POSITION order; pos_dev [N] int32: row id ->
 *   position (null = identity); cb_dev [M, 256, D / M] fp32, 1 <= M <= 64, D % M == 0, (D / M) % 16 == 0;
 *   list_offsets_dev [nlist + 1] int32, centroid_dev [nlist, D] fp32, nlist >= 1: all three or none (null, null, 0).  None: the codes
 *   are codes of the rows themselves.  Given: they are residual codes; the list of position p is the l with off[l] <= p < off[l + 1],
 *   and a position at or beyond off[nlist] is in no list;
 *   db_norm_dev [N] fp32 in ID order: required under L2, may be null under IP.
 * The row, with m = e / dsub, dsub = D / M:  xhat_j[e] = cb[m][code[pos(j)][m]][e - m dsub], for residual codes
 *   xhat_j[e] = centroid[l][e] + (that): ONE fp32 addition, rounded before it enters the chain (sylber_ivfpq_decode's row).  A row whose
 *   bad byte is set, and a residual-coded row in no list, is a NaN row: its local cost is +inf against every phrase row.
 * Everything else -- the ascending fmaf chain from 0 over e, local cost, recurrence, tie order, tracked start, padding, ranking, the
 * other arguments and the workspaces (sylber_dtw16_workspace_bytes(n_phrases, m, 1), sylber_dtw_align_workspace_bytes) -- is
 * sylber_dtw_rerank's and sylber_dtw_align's, word for word.  So the outputs of either equal those of the fp32 entry on the
 * materialised plane db_dev[j] = xhat_j (NaN rows as above) with the same db_norm_dev, BIT FOR BIT.
 * sylber_dtw_rerank_occurrences_codes: sylber_dtw_rerank_occurrences on the same coded database (PQSyllableIndex.search_occurrences and
 *   IVFPQSyllableIndex.search_occurrences with rerank=False): the arguments of sylber_dtw_rerank_codes, the coded-database group
 *   unchanged and in the same order; k as in sylber_dtw_rerank_occurrences (1 <= k <= 128, not bounded by m); workspace_dev:
 *   sylber_dtw_occ_workspace_bytes(n_phrases, m, k) bytes.  The outputs equal those of sylber_dtw_rerank_occurrences on the
 *   materialised plane db_dev[j] = xhat_j with the same db_norm_dev, BIT FOR BIT; NaN rows are a masked row, an out-of-range
 *   position and a residual-coded row in no list.  It also refuses n_phrases x m x k beyond 2^30 list entries.
 * Every index read from device memory is clamped before it is an address: stale pos_dev, offsets or windows give NaN rows or padding,
 * never an access outside the arrays.  Bad arguments (those of the fp32 entry, the geometry of M, a partial list group, a null
 * code_dev or cb_dev) return 1 with sylber_last_error before any device call. */
int sylber_dtw_rerank_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                            const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev, const uint8_t* bad_dev,
                            const int32_t* pos_dev, const float* cb_dev, int32_t M, const int32_t* list_offsets_dev,
                            const float* centroid_dev, int32_t nlist, int32_t N, int32_t D, const float* db_norm_dev, int32_t metric,
                            const int32_t* cand_dev, int32_t m, const int32_t* seq_offsets_dev, int32_t n_seq, int32_t k, float* cost_dev,
                            int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream);
int sylber_dtw_rerank_occurrences_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                        const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev, const uint8_t* bad_dev,
                                        const int32_t* pos_dev, const float* cb_dev, int32_t M, const int32_t* list_offsets_dev,
                                        const float* centroid_dev, int32_t nlist, int32_t N, int32_t D, const float* db_norm_dev,
                                        int32_t metric, const int32_t* cand_dev, int32_t m, const int32_t* seq_offsets_dev, int32_t n_seq,
                                        int32_t k, float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream);
int sylber_dtw_align_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                           const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev, const uint8_t* bad_dev,
                           const int32_t* pos_dev, const float* cb_dev, int32_t M, const int32_t* list_offsets_dev,
                           const float* centroid_dev, int32_t nlist, int32_t N, int32_t D, const float* db_norm_dev, int32_t metric,
                           const int32_t* pair_phrase_dev, const int32_t* pair_window_dev, int32_t n_pairs, int32_t max_cols,
                           int32_t max_rows, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* start_dev,
                           void* workspace_dev, void* stream);

/* Compressed phrase search (sylber_amd/pq.py: PQSyllableIndex.search_phrases): sylber_dtw16_scan with the database given as
 * product-quantization codes.  codes_dev [N, M] uint8 and bad_dev [N] uint8 (nullable; 1 = a masked row) as sylber_pq_encode writes
 * them; codebooks16_dev [M, 256, D / M] = sylber_knn16_pack of the fp32 codebooks in `storage`; 1 <= M <= 64, D % M == 0,
 * (D / M) % 16 == 0.  With x^_j = sylber_pq_decode(code_j), the coarse score is t(i, j) = fmaf(-2, dot16(q16_i, round16(x^_j)), c_j),
 * c_j = recon_norm_dev[j] under L2 (sylber_knn_row_norms of x^_j; may be null under IP), 0 under IP, and NaN in both metrics for a
 * masked row, whose local cost is therefore +inf against every phrase row.  round16 is element-wise, so round16(x^_j) is gathered
 * from codebooks16_dev and no row is ever materialised.  Everything else -- the other arguments, the local cost, the recurrence, the
 * candidates, cand_dev / coarse_dev, the workspace of sylber_dtw16_workspace_bytes(n_phrases, m, cuts) bytes -- is
 * sylber_dtw16_scan's: the outputs equal those of sylber_dtw16_scan on db16_dev = sylber_knn16_pack(x^) (a NaN row for a masked
 * one) with db_norm_dev = recon_norm_dev, bit for bit.  Bad arguments return 1 with sylber_last_error before any device call. */
int sylber_dtwpq_scan(const void* q16_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                      const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const uint8_t* codes_dev,
                      const uint8_t* bad_dev, const void* codebooks16_dev, int32_t N, int32_t D, int32_t M, const float* recon_norm_dev,
                      const float* q_norm_dev, int32_t metric, int32_t storage, int32_t m, const int32_t* seq_id_dev,
                      const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev,
                      int32_t* cand_dev, float* coarse_dev, void* workspace_dev, void* stream);

/* Phrase search through the inverted file, stage 1b (sylber_amd/search.py: SyllableIndex.search_phrases_seeded): per-row
 * neighbours ("seeds") vote for candidate sequences, which sylber_dtw_rerank then scores exactly.  seed_score_dev fp32 and
 * seed_id_dev int64, [R, seeds] each (1 <= seeds <= 128): what a search reports under `metric` for each of the R phrase rows,
 * concatenated in phrase order (NOT the packed blocks of sylber_dtw_plan); phrase_row_dev / phrase_len_dev [n_phrases]: first row and
 * length (1 .. 64) of each phrase; seq_offsets_dev [n_seq + 1]; the two group arrays both or neither.
 *   local cost of a seed: d = score (L2), d = max(0, 1 - score) (IP): the d of sylber_dtw_search, bit for bit.  A seed is ignored
 *   when its id is -1 (or outside [0, seq_offsets[n_seq])), its score is NaN or its d is +inf.
 *   Per phrase p with rows i = 0 .. m_p - 1: seq(j) = the sequence holding row j; floor_i = the largest d among row i's valid seeds
 *   (0 without one); best_i(s) = the smallest d among row i's valid seeds in sequence s (floor_i without one); s is SEEN when some
 *   row has a valid seed in it, and ADMISSIBLE unless seq_group[s] == phrase_group[p];
 *   bound(p, s) = (((0 + best_0) + best_1) + ... + best_{m_p - 1}), fp32 additions in ascending i.
 * cand_dev int32 [n_phrases, m] (1 <= m <= 128): the m smallest admissible seen sequences of finite bound under (bound, sequence
 * number), padded with -1; bound_dev fp32 [n_phrases, m]: their bounds, padded with +inf.  Every operation is an fp32 min, max or
 * add in a fixed order, so the outputs are unique: independent of the order of the seeds within a row, of duplicates, of how phrases
 * are launched and of what the outputs held.  When the seeds of every row are its `seeds` nearest rows (all of them: no exclusion
 * beyond whole sequences), bound(p, s) <= the sylber_dtw_search cost of (p, s), exactly.  One workgroup per phrase, everything in
 * LDS; no workspace.  Bad arguments return 1 with sylber_last_error before any device call. */
int sylber_phrase_vote(const float* seed_score_dev, const int64_t* seed_id_dev, int32_t seeds, const int32_t* phrase_row_dev,
                       const int32_t* phrase_len_dev, int32_t n_phrases, const int32_t* seq_offsets_dev, int32_t n_seq, int32_t metric,
                       const int32_t* phrase_group_dev, const int32_t* seq_group_dev, int32_t m, int32_t* cand_dev, float* bound_dev,
                       void* stream);

/* Learned quantizer (sylber/model/quantizer.py:6-77, 182-257: `load_quantizer` / `Quantizer`), eval, exact fp32.  The host
 * (sylber_amd/quantizer.py) chains: sylber_lq_norm (input norm / padding) -> sylber_ffenc -> sylber_lq_norm (output norm, blank rows)
 * -> sylber_rvq_assign for the art window and the pitch window -> sylber_lq_norm of the quantized rows.  All data pointers are device
 * pointers; `ld*` are row strides in elements.
 *
 * _unit_norm / _unit_norm_sep (quantizer.py:33-44) and the blank mask: y[r, c] = x[r, c] / sqrt(sum x[r, range]^2 + 1e-5) for c < D
 *   (normalize != 0; else a copy), the ranges [0, split) and [split, D) when 0 < split < D, else [0, D); y[r, D..Dy) = 0; the whole
 *   row 0 where the row of blank_dev (width D_blank, nullable) has no positive sum of squares.  In place needs ldx == ldy. */
int sylber_lq_norm(const float* x_dev, int64_t ldx, int32_t n, int32_t D, int32_t split, int32_t normalize, const float* blank_dev,
                   int64_t ld_blank, int32_t D_blank, float* y_dev, int64_t ldy, int32_t Dy, void* stream);
/* FFEncoder.forward (quantizer.py:15-31) on the exact-fp32 GEMM, one launch per Linear in upstream's order.  dims (host) [num_hidden + 2]:
 * the input width, the hidden widths, the output width, each padded to a multiple of 16; weights (host array of device pointers)
 * [2 * (3 * num_hidden + 1)]: (W, b) of mlp.{2i}, mlp.{2i+1}.0, mlp.{2i+1}.3 per hidden width, then of mlp.{2H}, each W [out][in] and
 * b [out] zero-padded to the padded widths.  x_dev [n][dims[0]], y_dev [n][dims[H+1]].
 *   workspace_dev: sylber_ffenc_workspace_floats(n, num_hidden, dims) floats */
int64_t sylber_ffenc_workspace_floats(int32_t n, int32_t num_hidden, const int32_t* dims);
int sylber_ffenc(const float* x_dev, int32_t n, int32_t num_hidden, const int32_t* dims, const float* const* weights, float* y_dev,
                 float* workspace_dev, void* stream);
/* Residual VQ of one group (GroupedResidualVQ, groups = 1, Euclidean codebooks), eval.  codebooks_dev [Q][Kp][Dp] with Kp = K rounded
 * up to 4 and Dp = D rounded up to 16, the padding zero; sqnorms_dev [Q][Kp] = ||row||^2, written once by sylber_rvq_prepare.
 * assign: r = x; per stage q: i_q = argmin_k ||r - E_q[k]|| (the arg-min of sylber_km_assign: ||e||^2 - 2 r.e, ties to the smallest k)
 *   into idx_dev[row * ld_idx + q], z += E_q[i_q] (z_dev nullable), r -= E_q[i_q].  x_dev / z_dev: windows of width D, strides ldx / ldz.
 *   workspace_dev: sylber_rvq_workspace_floats(n, K, D) floats.
 * decode: z = sum_q E_q[clamp(idx[row * ld_idx + q], 0, K - 1)] in stage order, the sums of assign bit for bit. */
int sylber_rvq_prepare(const float* codebooks_dev, int32_t Q, int32_t K, int32_t D, float* sqnorms_dev, void* stream);
int64_t sylber_rvq_workspace_floats(int32_t n, int32_t K, int32_t D);
int sylber_rvq_assign(const float* x_dev, int64_t ldx, int32_t n, int32_t D, const float* codebooks_dev, const float* sqnorms_dev, int32_t Q,
                      int32_t K, int32_t* idx_dev, int64_t ld_idx, float* z_dev, int64_t ldz, float* workspace_dev, void* stream);
int sylber_rvq_decode(const int32_t* idx_dev, int64_t ld_idx, int32_t n, const float* codebooks_dev, int32_t Q, int32_t K, int32_t D,
                      float* z_dev, int64_t ldz, void* stream);

/* N3: front half of SegmentSynthesis.resynthesize (sylber/model/segment_synthesis.py:103-140): segment means broadcast
 * back to their frames -> `MLP` conditioner (Linear -> RFF -> ... -> Linear, segment_synthesis.py:17-53) -> frames with
 * hidden-state norm < norm_thr zeroed.  HOST pointers to fp32 tensors in nn.Linear / nn.LayerNorm layout. */
#define SYLBER_MLP_MAX_HIDDEN 4
typedef struct {
    int32_t input_dim, output_dim, num_hidden;
    int32_t hidden_dims[SYLBER_MLP_MAX_HIDDEN];                 /* each 512 or 768 */
    struct {
        const float *lin_w, *lin_b;                             /* mlp.{2i}: Linear(in, dim) */
        const float *ff1_w, *ff1_b, *ff2_w, *ff2_b, *ln_w, *ln_b; /* mlp.{2i+1}: RFF.linear1 / linear2 / norm */
    } hidden[SYLBER_MLP_MAX_HIDDEN];
    const float *out_w, *out_b;                                 /* mlp.{2 num_hidden}: Linear(dim, output_dim) */
} SylberMlpWeights;
typedef struct sylber_mlp* sylber_mlp_t;
int sylber_mlp_create(const SylberMlpWeights* w, int device, sylber_mlp_t* out);
void sylber_mlp_destroy(sylber_mlp_t m);
int64_t sylber_condition_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S);
/* hidden_dev [B,T,D], seg_dev [B,T,2], nseg_dev [B], feat_dev [B,T,D]: the buffers of sylber_forward / sylber_segment;
 * S: segment slots per utterance to run through the MLP (max nseg <= S <= T);
 * avg_hidden_dev [B,T,D] (nullable): averaged_target_hidden_states; cond_dev [B,T,output_dim]: the conditioning input */
int sylber_condition(sylber_mlp_t m, const float* hidden_dev, const int64_t* seg_dev, const int32_t* nseg_dev, const float* feat_dev,
                     int32_t B, int32_t T, int32_t S, float norm_thr, float* avg_hidden_dev, float* cond_dev, float* workspace_dev,
                     void* stream);

/* syllable units -> conditioning input: the fused form of
 *   sylber_condition_features(expand_feature(decode(units), durations))   (flowmatching.py:873-882, segment_synthesis.py:135-140)
 * with the MLP run once per unit instead of once per frame; the result is bitwise the same.
 *   c1_dev [K1, input_dim], c2_dev [K2, input_dim] or NULL (one codebook); units_dev [B, S, ncb] int32 (ncb = 2 with c2, else 1),
 *   ids in [-1, K) (-1 reads as 0, KMQuantizer.decode's clip); spans_dev [B, S, 2] int32: unit j of row b covers frames
 *   [start, end), 0 <= start < end <= T, start >= the previous unit's end; nunits_dev [B] in [0, S]; frames_dev [B] in [1, T] or
 *   NULL (every row T frames).  cond_dev [B, T, output_dim]: frame t of row b takes the MLP row of the unit whose span holds it,
 *   0 where none does, where t >= frames[b], or where the unit's decoded row has sqrt(sum x^2) < 1e-4.
 *   All device pointers.  The tables are checked on the device before anything else runs (the call synchronises `stream` once);
 *   a bad entry returns an error naming the call.  workspace_dev: sylber_condition_units_workspace_floats(m, B, S) floats */
int64_t sylber_condition_units_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S);
int sylber_condition_units(sylber_mlp_t m, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2, const int32_t* units_dev,
                           const int32_t* spans_dev, const int32_t* nunits_dev, const int32_t* frames_dev, int32_t B, int32_t T, int32_t S,
                           float* cond_dev, float* workspace_dev, void* stream);
/* packed batches: the conditioning of each clip's own frames, back to back -- clip b's frame t is row F_b + t of cond_dev
 * [sum frames_host, output_dim] (F_b = frames_host[0] + ... + frames_host[b - 1]), the layout sylber_cfm_sample_packed reads.  Every row
 * is bitwise the padded call's (sylber_condition / sylber_condition_units with frames_dev) for the same clip.  frames_host [B] >= 1 and
 * offsets_host [B + 1] (sylber_packed_layout) are read before the call returns.  workspace_dev:
 * sylber_condition_packed_workspace_floats(m, B, S) floats (for both calls). */
int64_t sylber_condition_packed_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S);
/* hidden_dev [offsets[B], D]: sylber_forward_packed's rows, clip b's frame t at row offsets_host[b] + t; seg_dev [B, K, 2], nseg_dev [B],
 * feat_dev [B, K, D]: sylber_segment_packed's tables (K = their pitch, max frames <= K); S: segment slots per clip run through the MLP
 * (max nseg <= S <= K); avg_hidden_dev [sum frames, D] (nullable) and cond_dev [sum frames, output_dim] as sylber_condition's, per frame */
int sylber_condition_packed(sylber_mlp_t m, const float* hidden_dev, const int32_t* offsets_host, const int32_t* frames_host, int32_t B,
                            const int64_t* seg_dev, const int32_t* nseg_dev, const float* feat_dev, int32_t K, int32_t S, float norm_thr,
                            float* avg_hidden_dev, float* cond_dev, float* workspace_dev, void* stream);
/* sylber_condition_units with frames_dev = frames_host and T = max frames_host (the same table checks), cond_dev [sum frames, output_dim] */
int sylber_condition_units_packed(sylber_mlp_t m, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2, const int32_t* units_dev,
                                  const int32_t* spans_dev, const int32_t* nunits_dev, const int32_t* frames_host, int32_t B, int32_t S,
                                  float* cond_dev, float* workspace_dev, void* stream);
/* expand_feature(avg_fts, durations) (flowmatching.py:873-882) on the device: row b of out_dev [B, T, D] is feats_dev[b, 0] repeated
 * durations[b, 0, 0] times, then durations[b, 0, 1] zero rows, then unit 1 ...  durations_dev [B, S, 2] int32 >= 0; every row must
 * sum to T (upstream's torch.stack refuses ragged rows), else an error.  Synchronises `stream` once (the check);
 * workspace_dev: B * S + 1 int32 */
int sylber_expand_units(const float* feats_dev, const int32_t* durations_dev, int32_t B, int32_t S, int32_t D, int32_t T, float* out_dev,
                        int32_t* workspace_dev, void* stream);

/* ---- per-handle options ------------------------------------------------------------------------ */
/* Tuning / test overrides, scoped to ONE handle (nothing process-global).  SYLBER_OPT_GEMM_TILE: value < 0 restores the
 * automatic choice (0 is a tile id); the other keys: 0 = automatic.
 *   SYLBER_OPT_GEMM_TILE               tile configuration id of the bf16 GEMM launches (csrc/gemm_tiles.h:
 *                                      0 = 256x128, 3 = 128x128, 4 = 128x192, 10 = 256x256 8-wave, 11 = 256x192 8-wave;
 *                                      hand-scheduled K loops (csrc/gemm_asm.hip; a launch whose epilogue / K has no such
 *                                      instantiation falls back to 128x192): 80 = 256x256 4-wave, 90 = 256x192, 95 = 256x256
 *                                      8-wave, 85 / 91 / 97 = the same with a three-slot X ring, 51 / 57 = 91 / 97 on 192-row tiles, 86 = that ring on a 256x128 tile / four waves (91 also requests the fp32 residual rows of out-proj / FFN2 from
 *                                      inside its K loop when the launch has whole tiles; 96 = 91 without that), 60 = the 64-byte-row first cut;
 *                                      round 6: 5 / 6 = 128x128 / 128x192 on EIGHT waves (same bits; measured no gain for these kernels, forced only);
 *                                      the v_mfma_f32_16x16x32 family (csrc/gemm_asm16.hip; 16-bit-output and plain fp32 epilogues): 47 = tile 97's geometry, 46 = its 192-row
 *                                      sibling, 13 / 14 = 128x128 / 128x192 hipcc-scheduled on four waves, 15 / 16 = the same on eight waves.  On a 16-bit-output launch
 *                                      (conv1-5, FFN1) ANY forced id runs on the family member of the same shape class unless SYLBER_OPT_GEMM_MFMA16 = -1)
 *   SYLBER_OPT_ATTN_QUERIES_PER_WAVE   0 (default): the hand-scheduled key loop (csrc/attention.hip attention_asm_kernel, generated by
 *                                      tools/gen_attn_asm.py; bf16 / fp16 modes); 32 or 64: the compiler-scheduled kernels with that many
 *                                      queries per wave (its reference; split16 always runs the 32-query one)
 *   SYLBER_OPT_GEMM_PERSISTENT         0 (automatic): GEMM launches of more than one round run as persistent workgroups
 *                                      walking the tile list (4-wave kernels: two per CU; the 256x256 kernel: one per CU
 *                                      with cross-tile operand prefetch); k > 0: k workgroups per CU for the 4-wave
 *                                      kernels; k < 0: one workgroup per tile everywhere (A/B switch)
 *   SYLBER_OPT_FUSE_OUTPROJ_LN         1: the attention out-projection and the LayerNorm behind it run as ONE launch on
 *                                      full-row tiles (csrc/gemm_rowln.hip; bit-identical outputs) where the shape allows;
 *                                      0 / -1 (default): GEMM launch + LayerNorm launch (faster with two batches in flight)
 *   SYLBER_OPT_CONV0_VALU              1: conv layer 0 of the 16-bit modes on the VALU kernel instead of the matrix-pipe one (A/B switch)
 *   SYLBER_OPT_RESLN_PREFETCH          the K loops of the attention out-projection and FFN2 request the rows of the fp32 residual stream
 *                                      they update while they run (csrc/gemm_asm.hip, bit-identical outputs): 1..3 = fragment columns
 *                                      (of 3 per wave) prefetched, -1 = none (the epilogue loads them), 0 = the default (1: measured
 *                                      best with two batches in flight; 3 is best with one, profiles/r04_resln_prefetch.md)
 *   SYLBER_OPT_FP8_ATTENTION           SYLBER_FP8 only: 1 (and 0 = the default) = the attention core on MXFP8 operands too -- the q / k / v projection
 *                                      quantises its outputs (e4m3, one power-of-two scale per 32 features of q / k and per 32 keys of v),
 *                                      P is e4m3: BASELINE configs[4] as worded, whatever the batch shape (round 5: the q / k / v launch pads its rows
 *                                      up to whole 256-row tiles and does not store the padding); -1 = always the bf16 core (q, k, v, P in bf16)
 *   SYLBER_OPT_GEMM_TAIL               k > 0: a GEMM launch whose tile count is not a whole number of rounds of 256 persistent workgroups is split BY ROWS --
 *                                      the rows of the full rounds on the chosen tile, the remaining rows as a second launch on tile id k (bit-identical
 *                                      outputs: every element is one fp32 chain over K whatever tile computes it).  0 / -1 (default): one launch.  Measured
 *                                      not to pay (a small tile alone on a CU is no faster than a big one; csrc/gemm_bf16.hip gemm_plan): the partial
 *                                      rounds are handled by the 192-row tiles below; this stays as a test vehicle
 *   SYLBER_OPT_GEMM_H192               0 (default): the cost model may pick the 192-row siblings of the hand-scheduled tiles (ids 51 = 192x192, 57 = 192x256:
 *                                      a second tile HEIGHT, for launches whose 256-row tile count leaves a partial last round); -1: 256-row tiles only (A/B)
 *   SYLBER_OPT_GEMM_MFMA16             0 (default): the GEMMs with 16-bit outputs (conv1-5, FFN1: csrc/gemm_bf16.hip EPI_BF16) run on the v_mfma_f32_16x16x32 family of
 *                                      kernels (csrc/gemm_asm16.hip, tile ids 13 / 14 / 46 / 47: the instruction shape that is cheapest per FLOP under the package power
 *                                      cap, profiles/r06_mfma16_loop.md); a forced SYLBER_OPT_GEMM_TILE id is mapped to the member of the same shape class on these
 *                                      launches.  -1: those launches on the 32x32x16 kernels of the earlier rounds (A/B switch).  The two families group an output
 *                                      element's fp32 sum over K differently (32-k against 16-k blocks): results agree to fp32 rounding of the accumulator, not bit
 *                                      for bit -- WITHIN either setting results do not depend on the batch shape or the tile.
 *   SYLBER_OPT_GEMM_MODEL              which tiles the GEMM launches of this handle get (csrc/gemm_bf16.hip gemm_plan).  0 (default): the handle OWNS the chip -- one batch in
 *                                      flight, as in a synchronous Segmenter.__call__: a launch is charged its partial last round (measured per kernel
 *                                      family) and may use the 192-row tiles; 5: the handle SHARES the chip with another in-flight batch (bench.py's
 *                                      pipeline, ShardedSegmenter's two engines): the CUs a partial round leaves idle go to the other stream's
 *                                      kernels, whole-round accounting with the round-5 constants measured fastest there (8 x 60 s: 8.57 vs 8.78 ms
 *                                      per step; alone on the chip the same handle is 5 % slower with it).  Outputs are bit-identical either way.
 *                                      (6 = 0 without the lone-round rule of round 6 -- a launch of fewer tiles than CUs on the one-per-CU persistent tiles costs a full round --
 *                                      i.e. the tile choice of rounds 5-6a for small batches: A/B switch.)
 *   SYLBER_OPT_SEGMENT                 0 (default): sylber_segment as wide kernels -- frame norms, one workgroup per unbroken run of speech frames
 *                                      (independent instances of get_segment's two phases), compaction, pooling one wave per segment, all on all
 *                                      CUs; -1: one workgroup per utterance (rounds 1-5; bit-identical, A/B switch and reference)
 *   SYLBER_OPT_FP16_AUDIT              1: (re)start the fp16 headroom audit -- from now on every forward of a SYLBER_FP16 / SYLBER_MIXED16 handle scans each
 *                                      16-bit activation buffer right behind its producer and accumulates, per stage, the number of values AT the
 *                                      format's saturation value (+-65504: the fp16 modes clamp on conversion, they never produce infinities) and the
 *                                      largest magnitude seen; read with sylber_get_fp16_audit.  0 (default): off, nothing is launched.
 *   SYLBER_OPT_PER_UTTERANCE           1: batch-invariant encoder -- conv0's GroupNorm statistics of row b are taken over that row's own conv0 frames
 *                                      (lengths_host[b] - 10) / 5 + 1 instead of the padded length, so hidden[b, :T_b] (T_b = sylber_num_frames(
 *                                      lengths_host[b])) is bit-identical to a forward of that clip alone in every precision (SYLBER_FP8 with
 *                                      SYLBER_OPT_FP8_ATTENTION = -1: its fp8 attention core is chosen by batch shape).  Frames at or past T_b hold
 *                                      whatever the forward computes there; segment with sylber_segment_frames.  Works in graph mode (the counts
 *                                      are uploaded before every replay).  0 (default): the reference's statistics over the padded time axis. */
enum { SYLBER_OPT_GEMM_TILE = 1, SYLBER_OPT_ATTN_QUERIES_PER_WAVE = 2, SYLBER_OPT_GEMM_PERSISTENT = 3, SYLBER_OPT_FUSE_OUTPROJ_LN = 4,
       SYLBER_OPT_CONV0_VALU = 5, SYLBER_OPT_RESLN_PREFETCH = 6, SYLBER_OPT_FP8_ATTENTION = 7, SYLBER_OPT_GEMM_TAIL = 8, SYLBER_OPT_SEGMENT = 9, SYLBER_OPT_FP16_AUDIT = 10, SYLBER_OPT_GEMM_H192 = 11, SYLBER_OPT_GEMM_MODEL = 12, SYLBER_OPT_GEMM_MFMA16 = 13,
       SYLBER_OPT_PER_UTTERANCE = 14 };
int sylber_set_option(sylber_t h, int32_t key, int32_t value);
/* the audit's counters since SYLBER_OPT_FP16_AUDIT was last set (synchronises the device): names[i] (static strings: conv0 .. conv6, ln512,
 * proj_xpad, layernorm, q, k, v, context, ffn1), saturated[i] values clamped at +-65504, max_abs[i] largest magnitude; returns the number of
 * stages written (<= cap), 0 when the audit never ran, -1 on error.  A non-zero `saturated` means this checkpoint / input does not fit
 * IEEE half at that stage: use SYLBER_BF16 (8 exponent bits) or SYLBER_SPLIT16. */
int sylber_get_fp16_audit(sylber_t h, const char** names, uint32_t* saturated, float* max_abs, int32_t cap);

/* the `features is not None` branch of resynthesize (segment_synthesis.py:135-140): features_dev [rows, input_dim] frame
 * features supplied by the caller (e.g. decoded unit embeddings) -> cond_dev [rows, output_dim] = MLP(features), rows with
 * ((f**2).sum(-1))**.5 < 1e-4 zeroed (no 1e-8 under the root, threshold fixed at 1e-4, :136-137);
 * workspace_dev: sylber_condition_workspace_floats(m, rows, 1) floats */
int sylber_condition_features(sylber_mlp_t m, const float* features_dev, int32_t rows, float* cond_dev, float* workspace_dev,
                              void* stream);

/* ---- introspection used by parity tests and the benchmark ------------------------------------ */
/* run sylber_forward only up to a stage: 0 = all, 1 = conv stack, 2 = +projection/pos-conv/LN,
 * 3 + l = through encoder layer l.  The stage output is written to hidden_dev in place of the final
 * hidden states: stage 1 -> [B,T,512] conv features, otherwise [B,T,768].
 * Negative stages are taps inside the front half (the same launches as every forward, then a copy; never captured into a graph,
 * not available to sylber_forward_packed), all fp32:
 *   SYLBER_TAP_CONV0    conv layer 0 alone (GroupNorm + GELU applied): [B, R0, 512] with R0 = 64 * sylber_padded_frames(Lmax), every
 *                       row of the 16-bit buffer widened exactly (hi + lo for SYLBER_SPLIT16); rows at or past (Lmax - 10) / 5 + 1 are +0
 *   SYLBER_TAP_CONV(i)  = -(1024 + i), i = 1..6: conv layer i alone (GELU applied), the forward ends right behind its launch: [B, R_i, 512] with
 *                       R_i = sylber_padded_frames(Lmax) << (6 - i), every row of the layer's output buffer (16-bit buffers widened exactly, hi +
 *                       lo for SYLBER_SPLIT16; a device-to-device copy for SYLBER_FP32).  Utterance b's valid rows are [0, L_i) of its R_i rows,
 *                       L_i = (L_(i-1) - k_i) / 2 + 1 from L_0 = (Lmax - 10) / 5 + 1 (k_i = 3 for i <= 4, else 2); rows [L_i, R_i) hold whatever
 *                       the launch computes from the rows behind the previous layer's valid ones.  Rows [0, T) of SYLBER_TAP_CONV(6) are stage 1.
 *                       i = 0 and i >= 7 are refused
 *   SYLBER_TAP_PROJ     the projected residual stream x, frames at or past an utterance's valid count zeroed: [B, T, 768]
 *   SYLBER_TAP_POSCONV  x + GELU(pos-conv(x)), the input of the encoder LayerNorm: [B, T, 768]
 * Taps inside encoder layer l: stage SYLBER_TAP_LAYER(l, k) = -(8 (l + 1) + k) ends the forward after one launch of the layer and returns
 * frames [0, T) of every utterance as fp32 [B, T, W]; 16-bit buffers are widened exactly (hi + lo for SYLBER_SPLIT16):
 *   k = SYLBER_LTAP_QKV       after the q / k / v projection: q | k | v in natural order (head-major q / k and the key-permuted V^T
 *                             gathered back), q as stored, i.e. pre-scaled by log2(e) / 8 in the 16-bit modes            W = 2304
 *       SYLBER_LTAP_CTX       after the attention: the context                                                           W = 768
 *       SYLBER_LTAP_ATTN_SUM  after the out-projection: bias + residual added, the input of LayerNorm 1                  W = 768
 *       SYLBER_LTAP_LN1       after LayerNorm 1: the FFN's operand                                                       W = 768
 *       SYLBER_LTAP_FFN1      after FFN1 (GELU applied)                                                                  W = 3072
 *       SYLBER_LTAP_FFN2_SUM  after FFN2: bias + residual added, the input of LayerNorm 2 (whose output is stage 3 + l)  W = 768
 *   SYLBER_FP8: the MXFP8 buffers (q / k / v with SYLBER_OPT_FP8_ATTENTION on, the context, LayerNorm 1's output, FFN1's output) are
 *   dequantised exactly -- e4m3 x 2^(s - 127) is an fp32 value -- and returned as [B, T, 2 W]: the W values, then W floats that hold
 *   each element's own block exponent s - 127 (constant over 32 features; for v over 32 keys of a feature), so that the scale bytes
 *   are observable as well.  q is as stored: pre-scaled by 1 / 8 (the fp8 attention core applies log2(e) itself).  The fp32 sums
 *   (ATTN_SUM, FFN2_SUM) keep W = 768, and so does QKV with SYLBER_OPT_FP8_ATTENTION at -1 (bf16 buffers, W = 2304, q pre-scaled
 *   by log2(e) / 8).
 *   Refused for l >= num_layers and (like every stop stage) by sylber_forward_packed.
 * Any other negative stage (-4 .. -7, k = 6, 7) is refused. */
enum { SYLBER_TAP_CONV0 = -1, SYLBER_TAP_PROJ = -2, SYLBER_TAP_POSCONV = -3 };
enum { SYLBER_LTAP_QKV = 0, SYLBER_LTAP_CTX = 1, SYLBER_LTAP_ATTN_SUM = 2, SYLBER_LTAP_LN1 = 3, SYLBER_LTAP_FFN1 = 4, SYLBER_LTAP_FFN2_SUM = 5 };
#define SYLBER_TAP_LAYER(l, k) (-(8 * ((l) + 1) + (k)))
#define SYLBER_TAP_CONV(i) (-(1024 + (i)))
int sylber_set_stop_stage(sylber_t h, int32_t stage);
/* per-kernel device time of the last forward, measured with HIP events on the launch stream.
 * names/ms arrays of capacity cap; returns the number of entries (<=cap) or <0 on error. */
int sylber_set_profiling(sylber_t h, int32_t enable);
int sylber_get_profile(sylber_t h, const char** names, float* ms, int32_t cap);
/* graph mode (bf16 / fp8 handles): the second sylber_forward with the same (B, Lmax, wav_dev, hidden_dev) on a
 * non-default stream captures its ~110 launches into a hipGraph and later calls replay it — for launch-bound small
 * batches (one 3 s utterance: 1.5 ms eager).  Up to 8 shapes are cached per handle; disabling frees them. */
int sylber_set_graph_mode(sylber_t h, int32_t enable);
/* bytes of device workspace currently held by the handle */
int64_t sylber_workspace_bytes(sylber_t h);

/* ---- resynthesis decoder (sylber/model/flowmatching.py:474-824: Regressor + ConditionalFlowMatcherWrapperRegressor.sample) ----
 * The sylber_resynthesis.yaml geometry only: dim 512, depth 8, 8 heads x 64, dim_cond_emb 256, dim_in_proj 64, 16 register
 * tokens, conv kernel 31, ff_mult 4 (FF inner 1365), dim_out 14.  HOST pointers to fp32 tensors in the layout of the
 * Regressor's state_dict(); `precision`: SYLBER_BF16 (default), SYLBER_FP16 (the same launches on IEEE-half operands) or
 * SYLBER_FP32 (parity mode: exact-fp32 GEMMs and attention). */
#define SYLBER_CFM_DEPTH 8
typedef struct {
    const float *attn_gamma_w, *attn_gamma_b, *attn_beta_w, *attn_beta_b;  /* layers.i.2: AdaptiveRMSNorm to_gamma / to_beta [512,2048], [512] */
    const float *q_gamma, *k_gamma;                                        /* layers.i.3.{q,k}_norm.gamma [8,1,64] */
    const float *qkv_w, *out_w;                                            /* layers.i.3.to_qkv [1536,512], to_out [512,512] (no bias) */
    const float *ff_gamma_w, *ff_gamma_b, *ff_beta_w, *ff_beta_b;          /* layers.i.4 */
    const float *ff1_w, *ff1_b, *ff2_w, *ff2_b;                            /* layers.i.5.0 [2730,512] (value | gate), 5.3 [512,1365] */
} SylberCfmLayer;
typedef struct {
    const float *proj_in_w, *proj_in_b;             /* [64,14], [64] */
    const float *time_freq, *time_w, *time_b;       /* sinu_pos_emb.0.weights [256], sinu_pos_emb.1 [2048,512], [2048] */
    const float *to_embed_w, *to_embed_b;           /* [512, 384] over [proj_in(y), cond_emb, proj_in(cond)], [512] */
    const float *conv_w, *conv_b;                   /* conv_embed.dw_conv1d.0 [512,1,31], [512] */
    const float *register_tokens;                   /* transformer.register_tokens [16,512] */
    const float *rotary_inv_freq;                   /* transformer.rotary_emb.inv_freq [32] */
    SylberCfmLayer layers[SYLBER_CFM_DEPTH];
    const float *final_gamma;                       /* transformer.final_norm.gamma [512] */
    const float *to_pred_w;                         /* [14,512] (no bias) */
} SylberCfmWeights;
typedef struct sylber_cfm* sylber_cfm_t;
int sylber_cfm_create(const SylberCfmWeights* w, int device, int precision, sylber_cfm_t* out);
void sylber_cfm_destroy(sylber_cfm_t h);
/* bytes of caller-owned device workspace for a [B, T] call of sylber_cfm_sample / sylber_cfm_eval (-1 on error) */
int64_t sylber_cfm_workspace_bytes(sylber_cfm_t h, int32_t B, int32_t T);
/* art_dev [B,T,14] fp32 = sample(cond_emb_dev [B,T,256] fp32) with torchdiffeq's fixed-grid midpoint rule on
 * t = linspace(0, 1, steps) (steps 1..65; 1 returns y0), starting from y0_dev [B,T,14] (nullable: zeros), then
 * channel 12 divided by pitch_amp.  No mask: every row's frames 0..T-1 are ordinary frames (upstream's behaviour).
 * Enqueued on `stream`; no host synchronisation. */
int sylber_cfm_sample(sylber_cfm_t h, const float* cond_emb_dev, int32_t B, int32_t T, int32_t steps, const float* y0_dev,
                      float pitch_amp, float* art_dev, void* workspace_dev, void* stream);
/* batch-invariant sibling of sylber_cfm_sample: row b is sampled as a [1, frames_host[b]] call samples it -- the depthwise conv treats
 * frames at or past frames_host[b] as its zero padding, attention sees the 16 register tokens and the row's own frames only, and
 * art_dev[b, t] = 0 for t >= frames_host[b].  frames_host [B] in [1, T], read before the call returns.  Same workspace size. */
int sylber_cfm_sample_frames(sylber_cfm_t h, const float* cond_emb_dev, const int32_t* frames_host, int32_t B, int32_t T, int32_t steps,
                             const float* y0_dev, float pitch_amp, float* art_dev, void* workspace_dev, void* stream);
/* packed batches: no padding to the longest clip.  Clip b (frames_host[b] >= 1 frames) gets a decoder slot of round_up(16 + frames_host[b], 64)
 * rows -- 16 register rows, its frames, zero rows -- and the slots follow each other: slot b = rows [slot_offsets[b], slot_offsets[b + 1]).
 * The multiple of 64 keeps every attention key tile inside its own slot.  Host only, no GPU; fails (status 1) on B < 1, a count below 1
 * or slots totalling 2^24 rows or more.  slot_offsets: [B + 1] out. */
int sylber_cfm_packed_layout(const int32_t* frames_host, int32_t B, int32_t* slot_offsets);
/* bytes of caller-owned device workspace for a sylber_cfm_sample_packed call (-1 on error) */
int64_t sylber_cfm_workspace_bytes_packed(sylber_cfm_t h, const int32_t* frames_host, int32_t B);
/* sylber_cfm_sample_frames of a packed batch: cond_dev [sum frames, 256], y0_dev (nullable) and art_dev [sum frames, 14] hold each clip's
 * frames back to back (clip b from row frames_host[0] + ... + frames_host[b - 1]).  Clip b's art is bit-identical to sylber_cfm_sample_frames'
 * row b (and to the clip alone).  SYLBER_BF16 and SYLBER_FP16 handles only; a count below 1, B < 1, steps outside 1..65 and an fp32
 * handle return status 1 before any launch.  frames_host is read before the call returns. */
int sylber_cfm_sample_packed(sylber_cfm_t h, const float* cond_dev, const int32_t* frames_host, int32_t B, int32_t steps, const float* y0_dev,
                             float pitch_amp, float* art_dev, void* workspace_dev, void* stream);
/* one velocity evaluation v_dev [B,T,14] = Regressor(x_dev [B,T,14], t, cond_emb_dev) (test aid: localises errors) */
int sylber_cfm_eval(sylber_cfm_t h, const float* x_dev, float t, const float* cond_emb_dev, int32_t B, int32_t T, float* v_dev,
                    void* workspace_dev, void* stream);

/* ---- single-op entry points (unit parity tests; same kernels the forward path launches) ------ */
/* C[M,N] (fp32) = A[M,K] (fp32, cast to bf16) x W[N,K]^T (fp32, cast to bf16) + bias[N] (nullable); act: 0 none,
 * 1 gelu (the bf16 path's polynomial), 2 gelu (erf); precision: SYLBER_BF16 or SYLBER_FP8 (K % 128 == 0);
 * tile: -1 = automatic, else the tile configuration id to run (parity tests sweep every configuration), + 1000 k for a
 * persistent launch of k x 256 workgroups (9000 + id: never persistent) */
int sylber_op_linear(const float* a_dev, const float* w_dev, const float* bias_dev, float* c_dev, int32_t M,
                     int32_t N, int32_t K, int32_t act, int32_t precision, int32_t tile, void* stream);
/* the same contraction through the 16-bit output epilogue the conv layers and FFN1 use: c16_dev [M,N] bf16 words */
int sylber_op_linear16(const float* a_dev, const float* w_dev, const float* bias_dev, uint16_t* c16_dev, int32_t M,
                       int32_t N, int32_t K, int32_t act, int32_t precision, int32_t tile, void* stream);
/* one 3-tap stride-2 layer of the conv feature extractor (transformers modeling_hubert.py TP:160-175: Conv1d(512, 512, 3, stride 2,
 * bias=False) + GELU) as the 16-bit forward runs it: implicit GEMM over channels-last rows, chunk-major K order, 16-bit out.
 * x_dev [R, 512] fp32 rows (R >= 2 M + 1), w_host [512 out][512 in][3] fp32 in HOST memory (torch layout), y16_dev [M, 512] bf16 words */
int sylber_op_conv3(const float* x_dev, const float* w_host, uint16_t* y16_dev, int32_t R, int32_t M, int32_t tile, void* stream);
/* the residual GEMM of an encoder block (attention out-projection, FFN2; transformers modeling_hubert.py TP:361-397 reached from
 * sylber/model/sylber.py:122), in place: pre[M,N] (fp32) <- A[M,K] W[N,K]^T + bias + LayerNorm(pre), the LayerNorm re-derived per
 * element as ((pre - mean) * rstd) * gamma + beta from stats[M,2] = (mean, rstd) and gamma / beta [N] -- the form the forward
 * uses, where the previous LayerNorm launch stores only its 16-bit output and the row statistics; bf16 operands, tile as above */
int sylber_op_linear_resln(const float* a_dev, const float* w_dev, const float* bias_dev, float* pre_dev, const float* stats_dev,
                           const float* gamma_dev, const float* beta_dev, int32_t M, int32_t N, int32_t K, int32_t tile, void* stream);
/* MXFP8 quantiser used by SYLBER_FP8: x [R,K] fp32 -> data [R,K] e4m3 + E8M0 scales, one per 32 elements along K,
 * stored K-pair-major [K/64, R, 2] (K % 64 == 0; the layout the GEMM's scale fetch wants); the block scale is the
 * smallest power of two 2^e with amax <= 448 * 2^e, elements are x / 2^e rounded to nearest even */
int sylber_op_mx_quantize(const float* x_dev, int32_t R, int32_t K, uint8_t* data_dev, uint8_t* scale_dev, void* stream);
/* y = LayerNorm(x [+ res]) over the last dim D (512 or 768), eps 1e-5 */
int sylber_op_layernorm(const float* x_dev, const float* res_dev, const float* g_dev, const float* b_dev,
                        float* y_dev, int32_t M, int32_t D, void* stream);
/* softmax(q k^T / 8 + key mask) v ; q,k,v,o: [B,T,768] fp32 (12 heads x 64); valid_dev [B] int32;
 * queries_per_wave: 0 = automatic, 32 or 64; precision: SYLBER_BF16 (bf16 q, k, v, P) or SYLBER_FP8 (q, k, v quantised to MXFP8
 * -- e4m3 with one power-of-two scale per 32 features of q / k and per 32 keys of v -- and P to e4m3: BASELINE configs[4]) */
int sylber_op_attention(const float* q_dev, const float* k_dev, const float* v_dev, const int32_t* valid_dev,
                        float* o_dev, int32_t B, int32_t T, int32_t precision, int32_t queries_per_wave, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLBER_HIP_H */
