/* pcodec.h -- C ABI of libpcodec.so, the MI355X-native encode/decode hot path of
 * EIDOSLAB/ProgressiveCodec (ChannelProgresssiveWACNN.compress()/decompress()).
 *
 * Plain C: pointers, sizes and integer status codes only; no C++/torch types cross the
 * boundary.  Device pointers are HIP device pointers, `stream` arguments are hipStream_t
 * passed as void* (NULL = default stream).  Every function returns PC_OK (0) or a negative
 * PC_ERR_* code and never aborts.  Functions are re-entrant for distinct objects/buffers.
 *
 * Each entry point names the reference interface it replaces (paths under
 * /root/reference/src/compress).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 */
#ifndef PCODEC_H
#define PCODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PC_API __attribute__((visibility("default")))
#else
#define PC_API
#endif

enum {
    PC_OK = 0,
    PC_ERR_ARG = -1,        /* invalid argument / unsupported shape (reference: ValueError, entropy_models.py:214-224) */
    PC_ERR_INDEX = -2,      /* CDF index out of range (reference: assert, rans_interface.cpp:110-111) */
    PC_ERR_BUFFER = -3,     /* output buffer too small */
    PC_ERR_TRUNCATED = -4,  /* bitstream shorter than the symbols it should hold */
    PC_ERR_CDF = -5,        /* malformed CDF / pmf (reference: assert, ops.cpp:45; rans_interface.cpp:48-57) */
    PC_ERR_HIP = -6,        /* HIP runtime error (see pc_last_hip_error) */
    PC_ERR_NOMEM = -7,
    PC_ERR_STATE = -8,      /* object not ready (e.g. tables not set: "Uninitialized CDFs. Run update() first"), or busy: a codec object
                               serves one compress / decompress / forward call at a time (use one object per concurrent caller) */
    PC_ERR_MISSING = -9     /* state_dict tensor missing or wrong shape */
};

PC_API const char* pc_version(void);
/* Id of the numeric contract this build codes under (include/pc_math.h: PC_NUMERIC_CONTRACT_ID).  Byte strings are only decodable by a
 * build with the same id -- not by the reference's PyTorch path, nor by a build of another contract revision: the decoder re-derives
 * mu / scale / mask from decoded data, and one differently rounded float desynchronises rANS.  No reference counterpart (the reference
 * has no on-wire format and assumes encoder == decoder process). */
PC_API uint32_t pc_contract_id(void);
PC_API const char* pc_strerror(int code);
PC_API int pc_last_hip_error(void);

/* ---------------------------------------------------------------------------------------
 * Entropy coder (host).  rANS: 64-bit state, 32-bit words, 16-bit precision, 4-bit bypass.
 * ------------------------------------------------------------------------------------- */

/* Upper bound in bytes of one encoded stream of n symbols (worst case all-bypass). */
PC_API size_t pc_rans_bound(size_t n);

/* Replaces compressai.ans.RansEncoder.encode_with_indexes (cpp_exts/rans/rans_interface.cpp:193-204,
 * i.e. BufferedRansEncoder::encode_with_indexes :99-164 + flush :166-191).
 * cdfs is a dense [n_cdf][cdf_stride] int32 table (the module buffer `_quantized_cdf`),
 * cdf_sizes = `_cdf_length`, offsets = `_offset`.  Output bytes are identical to the reference's. */
PC_API int pc_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, size_t n,
                                       const int32_t* cdfs, int n_cdf, int cdf_stride,
                                       const int32_t* cdf_sizes, const int32_t* offsets,
                                       uint8_t* out, size_t out_cap, size_t* out_len);

/* Replaces compressai.ans.RansDecoder.decode_with_indexes (rans_interface.cpp:206-275). */
PC_API int pc_rans_decode_with_indexes(const uint8_t* encoded, size_t encoded_len,
                                       const int32_t* indexes, size_t n,
                                       const int32_t* cdfs, int n_cdf, int cdf_stride,
                                       const int32_t* cdf_sizes, const int32_t* offsets,
                                       int32_t* symbols_out);

/* Replaces compressai.ans.RansDecoder.set_stream + decode_stream (rans_interface.cpp:277-350): one stream decoded in several calls
 * (each with its own indexes / tables).  `state` is two uint64 owned by the caller: zero both before the first call on a stream (that
 * call reads the stream's initial state, as set_stream does); every successful call advances them.  The reference keeps this state
 * inside the decoder object; here it stays with the caller so the function is re-entrant.
 * compressai.ans.BufferedRansEncoder (encode_with_indexes ... flush, rans_interface.cpp:99-191) needs no entry point of its own:
 * its output is by construction that of ONE pc_rans_encode_with_indexes call over the concatenated symbols / indexes. */
PC_API int pc_rans_decode_stream(const uint8_t* encoded, size_t encoded_len, uint64_t* state,
                                 const int32_t* indexes, size_t n,
                                 const int32_t* cdfs, int n_cdf, int cdf_stride,
                                 const int32_t* cdf_sizes, const int32_t* offsets,
                                 int32_t* symbols_out);

/* Batched forms: n_streams independent streams of n symbols each (one per image, as the loop at
 * entropy_models.py:227-235 / :276-286 produces), coded on a host thread pool.
 * symbols/indexes: [n_streams][n].  Encode writes stream s at out + s*out_stride. */
PC_API int pc_rans_encode_batch(const int32_t* symbols, const int32_t* indexes, size_t n_streams, size_t n,
                                const int32_t* cdfs, int n_cdf, int cdf_stride,
                                const int32_t* cdf_sizes, const int32_t* offsets,
                                uint8_t* out, size_t out_stride, size_t* out_lens, int n_threads);
PC_API int pc_rans_decode_batch(const uint8_t* const* encoded, const size_t* encoded_lens, size_t n_streams,
                                const int32_t* indexes, size_t n,
                                const int32_t* cdfs, int n_cdf, int cdf_stride,
                                const int32_t* cdf_sizes, const int32_t* offsets,
                                int32_t* symbols_out, int n_threads);

/* The decoder's fast form of pc_rans_decode_batch: CDF indexes as bytes (n_cdf <= 256; the GaussianConditional has 64 rows), a per-row
 * start table instead of the reference's linear scan (rans_interface.cpp:238-241), two streams per host thread in lock step.  Same
 * symbols, same error codes. */
PC_API int pc_rans_decode_batch_u8(const uint8_t* const* encoded, const size_t* encoded_lens, size_t n_streams,
                                   const uint8_t* indexes, size_t n,
                                   const int32_t* cdfs, int n_cdf, int cdf_stride,
                                   const int32_t* cdf_sizes, const int32_t* offsets,
                                   int32_t* symbols_out, int n_threads);

/* Replaces compressai._CXX.pmf_to_quantized_cdf (cpp_exts/ops/ops.cpp:10-67).  cdf_out has n+1 entries. */
PC_API int pc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* cdf_out);

/* ---------------------------------------------------------------------------------------
 * Device stages (asynchronous on `stream`).  Activations are NHWC float32.
 * ------------------------------------------------------------------------------------- */

/* Generic convolution / transposed convolution / linear layer with the reference's weight layout.
 *   kind 0: nn.Conv2d weight [Cout][Cin][k][k], stride s, padding k/2   (models/utils.py:186, layers/layers.py:15,27)
 *   kind 1: nn.ConvTranspose2d(k=5, s=2, p=2, output_padding=1) weight [Cin][Cout][5][5]   (models/utils.py:196)
 *   kind 2 (pc_pack_conv_weight only): the same transposed conv with Cout = 3, k = 5 and Cin % 16 == 0 rewritten as the codec's sub-pixel
 *           output layer -- a 3x3 stride-1 conv with 12 channels n = c*4 + py*2 + px, PixelShuffle(2) in the store; 9 * 12 * Cin floats
 * `w_packed` must come from pc_pack_conv_weight (tap-major; the layout -- [taps][Cin][Cout] or [taps][Cout][Cin] -- is a
 * function of (kind, Cin, Cout, k) only).
 * act: 0 none, 1 GELU.  x: [B][H][W][Cin], out: [B][Ho][Wo][Cout]. */
PC_API int pc_pack_conv_weight(const float* w_host, int kind, int Cout, int Cin, int k, float* w_packed_host);
PC_API int pc_conv2d_nhwc(const float* x, int B, int H, int W, int Cin,
                          const float* w_packed, const float* bias, int kind, int Cout, int k, int stride,
                          int act, int tile_cfg, float* out, void* stream);

/* GDN / IGDN (layers/gdn.py:50-63) with already re-parametrised beta [C] and gamma [C_out][C_in] (the module's own layout). */
PC_API int pc_gdn_nhwc(const float* x, int B, int H, int W, int C, const float* beta, const float* gamma,
                       int inverse, float* out, void* stream);

/* Shifted-window attention core between the qkv and proj Linears (layers/win_attention.py:84-115,153-207).
 * qkv: [B][H][W][3C]; bias: dense [heads][T][T]; out: [B][H][W][C]. */
PC_API int pc_win_attention_nhwc(const float* qkv, const float* bias, int B, int H, int W, int C, int heads,
                                 int window, int shift, float* out, void* stream);

/* ChannelMask "point-based-std" threshold (layers/masking.py:205-223): thr[b] = torch.quantile(scale[b].ravel(), q).
 * scale: [B][HW][C] with pixel stride ld. */
PC_API int pc_mask_quantile_threshold(const float* scale, int ld, int B, int HW, int C, float q, float* thr, void* stream);

/* Fused mask -> index -> quantise -> dequantise of one 32-channel slice (encoder side):
 *   mask = scale >= thr[b]                      (masking.py:219; mask_mode 1; 0 = no mask, 2 = ones, 3 = zeros)
 *   idx  = build_indexes(scale * mask)          (entropy_models.py:661-666; CHProg_cnn.py:751,828)
 *   sym  = int(round((y [- ybase] - mu) [* mask]))   (entropy_models.py:137-150; CHProg_cnn.py:752,780-781,830)
 *   yhat = float(sym) + mu                      (CHProg_cnn.py:754-755,833-834)
 * scale/mu/y/ybase/yhat NHWC with their own pixel strides; sym/idx/mask out in [B][32][HW] (rANS order). */
PC_API int pc_gc_prep_encode(const float* scale, int ld_scale, const float* mu, int ld_mu,
                             const float* y, int ld_y, const float* ybase, int ld_ybase,
                             const float* thr, int mask_mode, int B, int HW,
                             const float* scale_table, int n_table, float scale_bound,
                             int32_t* sym, int32_t* idx, float* mask, float* yhat, int ld_yhat, void* stream);
PC_API int pc_gc_prep_decode_index(const float* scale, int ld_scale, const float* thr, int mask_mode, int B, int HW,
                                   const float* scale_table, int n_table, float scale_bound,
                                   int32_t* idx, float* mask, void* stream);
PC_API int pc_gc_dequantize(const int32_t* sym, const float* mu, int ld_mu, int B, int HW,
                            float* yhat, int ld_yhat, void* stream);

/* ---------------------------------------------------------------------------------------
 * The codec object: ChannelProgresssiveWACNN (models/CHProg_cnn.py:30) in the canonical
 * configuration, weights resident in HBM, compress()/decompress() as native launch sequences.
 * ------------------------------------------------------------------------------------- */
typedef struct pc_codec pc_codec;

enum { PC_MASK_POINT_BASED_STD = 0, PC_MASK_TWO_LEVELS = 1, PC_MASK_THREE_LEVELS_STD = 2 };   /* layers/masking.py:205-247 */
enum { PC_F32 = 0, PC_I32 = 1, PC_I64 = 2 };

PC_API int pc_codec_create(pc_codec** out, int device);
PC_API void pc_codec_destroy(pc_codec* c);

/* load_state_dict (models/cnn.py:195-202): one call per reference state_dict key, host pointers.
 * Unknown keys are ignored (returns PC_OK); shape mismatches return PC_ERR_MISSING. */
PC_API int pc_codec_set_tensor(pc_codec* c, const char* name, const void* data, int dtype,
                               const int64_t* shape, int ndim);
/* Entropy tables: the module buffers _quantized_cdf/_cdf_length/_offset after update() (models/cnn.py:137-142). */
PC_API int pc_codec_set_tables(pc_codec* c, int which /*0 = gaussian_conditional, 1 = entropy_bottleneck*/,
                               const int32_t* cdf, int n_cdf, int cdf_stride, const int32_t* cdf_sizes,
                               const int32_t* offsets);
/* update(scale_table=...) (models/cnn.py:137-142 -> GaussianConditional.update_scale_table, entropy_models.py:588-597): replace the
 * table of scales build_indexes searches (2..64 ascending floats, host pointer); set the matching CDFs with pc_codec_set_tables.
 * Only after pc_codec_finalize. */
PC_API int pc_codec_set_scale_table(pc_codec* c, const float* table, int n);
/* Validate that every tensor is present, fold the GDN re-parametrisation, pack weights into HBM. */
PC_API int pc_codec_finalize(pc_codec* c);
PC_API int pc_codec_set_threads(pc_codec* c, int n_threads);
/* Schedule options of one codec object -- how the launch sequence is laid over streams and host threads, never what it computes (every
 * byte string and x_hat is identical under every setting).  No reference counterpart (the reference is one stream, one thread).
 *   "serial_schedule" 0 / 1   1: the whole chain on the caller's stream, one batch lane, no base || enhancement pipelining -- the form a
 *                             profiler wants (a launch's duration is its own); default 0
 *   "lanes_enc", "lanes_dec"  0 (default: 1 / 2) .. 8: sub-batches of compress / decompress that run on streams of their own
 *   "host_threads"            as pc_codec_set_threads
 *   "profile_in_schedule" 0/1 1: pc_codec_profile_begin only brackets the launches and leaves the schedule alone (default 0: profiling
 *                             forces the serial schedule so that a launch's duration is its own)
 *   "group_siblings" 0 / 1    1 (default): sibling convolutions of identical shape share launches -- layer 1 of the hyper-synthesis nets
 *                             as one wide layer, their layers 2-5 as scale || mean pairs, and unit k of the two branches of a
 *                             window-attention module at small M as one grouped unit; 0: one launch per layer (for A/B timing)
 * Unknown names and out-of-range values return PC_ERR_ARG.  The conv kernel's tuning switches (PC_CONV_*) exist only in the -DPC_TUNING
 * build of the library (csrc/Makefile `tuning`), not here. */
PC_API int pc_codec_set_option(pc_codec* c, const char* name, int value);
/* How the host entropy-coding pool of this process is laid out: threads = min(16, CPUs allowed by affinity and cgroup quota / local ranks),
 * pinned -- when there are several local ranks (LOCAL_WORLD_SIZE / LOCAL_RANK) -- to this rank's contiguous slice of the allowed CPUs
 * starting at first_cpu.  No reference counterpart (the reference codes on one thread under the GIL, entropy_models.py:226-235). */
PC_API int pc_host_pool_plan(int* n_threads, int* first_cpu, int* n_allowed);

/* compress (models/CHProg_cnn.py:686-847).  x: device, NCHW [B][3][H][W], H and W multiples of 64.
 * On success the codec holds n_slices*B + B byte strings (n_slices = 10 for quality <= 0, else 20) until
 * the next call; masks_out (device, [10][B][32][H/16][W/16], may be NULL) receives the "masks" entry. */
PC_API int pc_codec_compress(pc_codec* c, const float* x, int B, int H, int W, double quality, int mask_pol,
                             float* masks_out, void* stream);
/* cust_map of compress() / decompress() (CHProg_cnn.py:686,849 -> layers/masking.py:171-194): device tensor NCHW
 * [B][320][H/16][W/16]; when set, the NEXT compress / compress_levels / decompress / decompress_levels call thresholds this map
 * (top quality*10 % per image and slice; quality >= 10 all, 0 none, whatever the mask policy) instead of the scale, then the
 * pointer is cleared.  NULL clears it. */
PC_API int pc_codec_set_cust_map(pc_codec* c, const float* cust_map);
/* The REM model family -- PostRateProcessedNetwork (models/CHProgREM.py:205; compress :673, decompress :896): a frozen base codec whose
 * predicted scale of every enhancement slice is refined by a LatentRateReduction CNN (:12-86, apply_latent_enhancement :375-428) chosen
 * by the range [check_levels[k], check_levels[k+1]) the quality falls in.  The CNN weights are state-dict tensors named
 * "post_latent.<level>.<slice>.<subnet>.<block>.{conv1,conv2,skip}.{weight,bias}" set with pc_codec_set_tensor before
 * pc_codec_finalize.  n_levels in 1..3 switches the refinement on for the following compress / decompress / forward calls, 0 switches it
 * off (plain ChannelProgresssiveWACNN).  mu_std (:30,42,397-416) and dimension ("big" / "middle", :23-43) are properties of the loaded
 * post_latent tensors (their names and shapes); checkpoint_rep is handed over with pc_codec_set_rem_checkpoint below. */
PC_API int pc_codec_set_rem(pc_codec* c, const double* check_levels, int n_levels);
/* checkpoint_rep of PostRateProcessedNetwork.compress / decompress (models/CHProgREM.py:676,773 / :901,989): a device tensor NCHW
 * [B][320][H/16][W/16] that replaces the decoded base slices as the x_base input of the LatentRateReduction nets in the NEXT compress /
 * decompress call, then the pointer is cleared (what the escalation mode chains from check level to check level, :335-373).  NULL clears. */
PC_API int pc_codec_set_rem_checkpoint(pc_codec* c, const float* checkpoint_rep);
/* ChannelProgresssiveWACNN(u_net_post = mode) (models/CHProg_cnn.py:87-88, 277-284): the UNet post-filter (layers/unet.py) behind the
 * synthesis transform.  mode 1: refine = Sequential(UNet(3, 16), conv3x3(16, 3)), tensors "refine.0.<unet>..." and "refine.1.{weight,bias}";
 * mode 2: two such nets "refine.<i>.0..." / "refine.<i>.1...", of which the decode paths use refine[1] (refine[0] serves only the training
 * forward, out of scope; its weights are loaded all the same).  Call before pc_codec_finalize, which then fails (PC_ERR_MISSING) if a
 * refine tensor is absent; 0 (the default) is no filter.  Every decode path (decompress, _levels, _packed, forward) then returns
 * clamp01(refine(clamp01(g_s(y_hat)))) on the padded image -- except under REM (pc_codec_set_rem n > 0), whose reference calls g_s
 * directly (models/CHProgREM.py:977,1123).  Encoder output does not change. */
PC_API int pc_codec_set_post_filter(pc_codec* c, int mode);
/* The topology switches of ChannelProgresssiveWACNN (models/CHProg_cnn.py:29-49) beyond the canonical configuration.  Every field's
 * zero is the canonical value, so a zero-initialised struct (the object's default) is multiple_hyperprior = delta_encode = True,
 * joiner_policy "res", support_progressive_slices 5 and the other switches False.
 *   support_deficit      5 - support_progressive_slices (0..5): determine_support keeps the last min(S, i) enhancement entries (:377-383)
 *                        and the prog stacks are 320 + 32 min(i+1, S+1) / LRP 320 + 32 min(i+2, S+2) channels wide (:235-274)
 *   no_delta_encode      delta_encode = False: the enhancement slice is coded without subtracting the raw base slice (:780-781)
 *   single_hyperprior    multiple_hyperprior = False: one h_mean_s / h_scale_s pair with 640 outputs, keys h_mean_s.<layer> (:705-715)
 *   joiner_cond          joiner_policy "cond": merge = joiner[i](cat(enhanced slice, base slice i)), keys joiner.<i>.{0,2,4} (:117-126,385-393)
 *   all_scalable         mean / scale support from mu_total / std_total instead of the merged slices (:784-785)
 *   total_mu_rep         mu_total holds mu + y_hat_base[i] (:801-810)
 *   support_std          std_total holds the raw scale instead of mu_total's entry (:802-805)
 *   residual_before_lrp  forward only: merge before the LRP (:1153-1164)
 * Call before pc_codec_finalize (PC_ERR_STATE after it, or on a WACNN object); PC_ERR_ARG for a field out of range.  The tensors
 * finalize expects follow the topology.  Results of the canonical topology never change. */
typedef struct pc_topology {
    int support_deficit;
    int no_delta_encode;
    int single_hyperprior;
    int joiner_cond;
    int all_scalable;
    int total_mu_rep;
    int support_std;
    int residual_before_lrp;
} pc_topology;
PC_API int pc_codec_set_topology(pc_codec* c, const pc_topology* t);
/* refine(x) (mode 1, which 0) or refine[which](x) (mode 2), unclamped: x and out device NCHW float [B][3][H][W], out may be x.  H and W
 * must be multiples of 4 (PC_ERR_ARG otherwise, where the reference fails in torch.cat); PC_ERR_STATE without a filter.  Scratch: 864
 * bytes per pixel of the batch, kept by the object (section 6 of DESIGN.md). */
PC_API int pc_codec_post_filter(pc_codec* c, int which, const float* x, int B, int H, int W, float* out, void* stream);
/* The single-rate model WACNN (models/cnn.py:23-340; "cnn" in the reference's registry, models/__init__.py) -- the "base" anchor curve
 * of the paper (training/train.py:379-380).  pc_codec_set_model(c, PC_MODEL_WACNN) before pc_codec_finalize switches the object to that
 * model's state dict: g_a.<layer> (3 -> 320), g_s.<layer>, h_a.0 = conv3x3(320, 320), h_mean_s.<layer> / h_scale_s.<layer> (one pair,
 * not a ModuleList), the ten cc_mean / cc_scale / lrp stacks, the EntropyBottleneck and GaussianConditional buffers; finalize returns
 * PC_ERR_MISSING if one is absent.  PC_MODEL_CHANNEL (the default) is ChannelProgresssiveWACNN.  PC_ERR_STATE after finalize, or for
 * PC_MODEL_WACNN with a post-filter set.  The progressive entry points (compress, _levels, decompress, _levels, _packed, forward,
 * post_filter, set_rem, set_cust_map, set_rem_checkpoint) return PC_ERR_STATE on a WACNN object, the pc_codec_wacnn_* ones on a
 * ChannelProgresssiveWACNN object.  The schedule options keep their meaning for the encoder chain (serial_schedule, lanes_enc) and do
 * not apply to the decoder, which decodes one stream on the caller's stream and thread; no byte or x_hat depends on them. */
enum { PC_MODEL_CHANNEL = 0, PC_MODEL_WACNN = 1 };
PC_API int pc_codec_set_model(pc_codec* c, int kind);
/* WACNN.compress (cnn.py:214-271): x device NCHW [B][3][H][W], H and W multiples of 64.  Leaves ONE y string for the whole batch --
 * every symbol of every slice and image in one BufferedRansEncoder stream, slice-major, then image, then C,H,W -- read with
 * pc_codec_get_string(c, 0, 0, ...), and B z strings (slice = -1).  pc_codec_num_slices returns 1. */
PC_API int pc_codec_wacnn_compress(pc_codec* c, const float* x, int B, int H, int W, void* stream);
/* WACNN.decompress (cnn.py:293-340): y = the batch's y string, z_strings / z_lens: B strings, zh, zw = "shape"; x_hat device NCHW
 * [B][3][64*zh][64*zw], clamped to [0,1].  A y string that does not end exactly where the batch's symbols do (another batch size or
 * shape, truncated or damaged) returns PC_ERR_TRUNCATED; the check is on the host, after the stream has been decoded. */
PC_API int pc_codec_wacnn_decompress(pc_codec* c, const uint8_t* y, size_t y_len, const uint8_t* const* z_strings, const size_t* z_lens,
                                     int B, int zh, int zw, float* x_hat, void* stream);
/* WACNN.forward in eval mode (cnn.py:145-192): x_hat device [B][3][H][W] = g_s(y_hat) UNCLAMPED, y_lik [B][320][H/16][W/16],
 * z_lik [B][192][H/64][W/64]; y_hat and z_hat are those of compress.  Needs the entropy_bottleneck._matrix/_bias/_factor tensors. */
PC_API int pc_codec_wacnn_forward(pc_codec* c, const float* x, int B, int H, int W, float* x_hat, float* y_lik, float* z_lik, void* stream);
PC_API int pc_codec_num_slices(const pc_codec* c);
/* string of y slice `slice` (0..n_slices-1) or of z (slice = -1) for image b */
PC_API int pc_codec_get_string(const pc_codec* c, int slice, int b, const uint8_t** data, size_t* len);

/* decompress (models/CHProg_cnn.py:849-999).  y_strings: [n_slices][B] pointers (slice-major), z_strings: [B];
 * zh, zw = "shape"; x_hat: device NCHW [B][3][64*zh][64*zw]. */
PC_API int pc_codec_decompress(pc_codec* c, const uint8_t* const* y_strings, const size_t* y_lens, int n_slices,
                               const uint8_t* const* z_strings, const size_t* z_lens, int B, int zh, int zw,
                               double quality, int mask_pol, float* x_hat, void* stream);

/* Multi-level ("progressive") coding of one batch -- SURVEY.md section 8(f) rank 1.  The reference's harness calls
 * compress() / decompress() once per mask level (training/step.py:322-337), recomputing g_a, h_a, the hyper-latent strings,
 * h_s and the ten base slices (CHProg_cnn.py:692-767 / :855-904) although none of them depends on the level.  These entry
 * points compute that shared part once and run only the enhancement chain (:775-845 / :930-983) and the synthesis transform
 * per level.  Every string, mask and x_hat is identical, bit for bit, to what n_levels separate pc_codec_compress /
 * pc_codec_decompress calls return.
 *   string slots: slice 0..9 = base (shared), slice 10..19 of level l = slot 10 + 10*l + (slice-10); a level with
 *   quality <= 0 has no enhancement strings.  masks_out: NULL or n_levels device pointers ([10][B][32][H/16][W/16] each, NULL
 *   allowed per level; untouched for quality <= 0).  x_hat: device, [n_levels][B][3][64*zh][64*zw]. */
PC_API int pc_codec_compress_levels(pc_codec* c, const float* x, int B, int H, int W, const double* qualities, int n_levels,
                                    int mask_pol, float* const* masks_out, void* stream);
/* string of level `level`: slice -1 = z, 0..9 = base (the same for every level), 10..19 = that level's enhancement */
PC_API int pc_codec_get_level_string(const pc_codec* c, int level, int slice, int b, const uint8_t** data, size_t* len);
/* y_strings / y_lens: [(10 + 10*n_levels) * B] in slot order (slot-major, then image); slots of quality-0 levels are ignored */
PC_API int pc_codec_decompress_levels(pc_codec* c, const uint8_t* const* y_strings, const size_t* y_lens,
                                      const uint8_t* const* z_strings, const size_t* z_lens, int B, int zh, int zw,
                                      const double* qualities, int n_levels, int mask_pol, float* x_hat, void* stream);

/* Bulk string transfer (binding overhead: 672 strings per Config-2 batch).  After a compress: _strings_size gives the total byte count
 * and the number of strings (all y slots, images inside a slot, then the z strings); _copy_strings concatenates them into dst (cap bytes)
 * and writes their lengths (lens_cap = entries available in lens; PC_ERR_BUFFER if either buffer is too small).  _decompress_packed takes the same layout: y strings of slots 0 .. 10+10*n_levels-1 (B each; empty strings
 * for the slots of quality-0 levels), then B z strings. */
PC_API int pc_codec_strings_size(const pc_codec* c, size_t* total_bytes, int* n_strings);
PC_API int pc_codec_copy_strings(const pc_codec* c, uint8_t* dst, size_t cap, size_t* lens, size_t lens_cap);
PC_API int pc_codec_decompress_packed(pc_codec* c, const uint8_t* data, const size_t* lens, int B, int zh, int zw,
                                      const double* qualities, int n_levels, int mask_pol, float* x_hat, void* stream);

/* forward_single_quality in eval mode (models/CHProg_cnn.py:1002-1198) -- SURVEY.md section 8(f) rank 2: the rate-estimation path
 * behind test_epoch / valid_epoch (training/step.py:215-267).  Runs the encoder chain without entropy coding and returns the
 * likelihood tensors: y_lik device [B][320 or 640][H/16][W/16] (640 when quality != 0), z_lik device [B][192][H/64][W/64],
 * x_hat device [B][3][H][W] (identical to decompress(compress(x))), masks_out as in pc_codec_compress (may be NULL).
 * force_enhanced != 0 with quality == 0 (:1006,1022,1064): both hyper-priors and the enhancement chain run with all-zero masks
 * (every enhancement symbol 0), y_lik has 640 channels and x_hat comes from the enhancement synthesis g_s[1].
 * Needs the entropy_bottleneck._matrix/_bias/_factor tensors in the state dict (PC_ERR_STATE otherwise). */
PC_API int pc_codec_forward(pc_codec* c, const float* x, int B, int H, int W, double quality, int mask_pol, float* x_hat,
                            float* y_lik, float* z_lik, float* masks_out, int force_enhanced, void* stream);

/* Measurement aid (bench.py roofline leg): while profiling is on, every launch of the MFMA convolution kernel made by
 * compress()/decompress() is bracketed by HIP events on the call's stream; _end returns the launch count, the summed
 * event time and the algorithmic FLOPs (2*M*N*K per launch, no padding counted). */
PC_API int pc_codec_profile_begin(pc_codec* c);
PC_API int pc_codec_profile_end(pc_codec* c, int64_t* n_launches, double* total_ms, double* total_flops);
/* algorithmic HBM bytes (every operand of a launch once: input, weights, bias, output, aux tensors) summed over the launches recorded
 * since pc_codec_profile_begin; read it after pc_codec_profile_end */
PC_API int pc_codec_profile_bytes(const pc_codec* c, double* total_algorithmic_bytes);
/* In-schedule profile (option "profile_in_schedule"): the bracketed launches of one or several codec objects -- e.g. the encoder and the
 * decoder object of progressivecodec_amd.CodecPipeline, which keep ~2.5 conv kernels in flight -- on ONE timeline.  pc_profile_set_epoch
 * drains `device` and records the epoch; after pc_codec_profile_end, pc_codec_profile_intervals returns every recorded launch's start / end
 * (ms since the epoch) and algorithmic FLOPs (cap entries available; all three arrays NULL: only *n is written).  bench.py folds the
 * intervals of both objects: FLOPs / (time during which at least one conv kernel runs) = the in-situ MFMA fraction of the schedule it
 * timed.  Measurement aids; no reference counterpart. */
PC_API int pc_profile_set_epoch(int device);
PC_API int pc_codec_profile_intervals(const pc_codec* c, double* t0_ms, double* t1_ms, double* flops, size_t cap, size_t* n);
/* Host entropy-coding figures of the object's last compress / decompress call ("rANS: report Msym/s per stream
 * and streams in flight"; no reference counterpart -- the reference times decompress() as a whole, training/step.py:332-340).
 * out[0] wall ms of the last compress call, out[1] host ms spent in rANS encoding during it (mostly hidden behind the GPU chain),
 * out[2] of those, the ms of the last pass that nothing hides ("exposed"), out[3] host ms of rANS decoding in the last decompress call
 * summed over the decoder's lanes (each slice's decode sits between two GPU steps of its chain), out[4] / out[5] symbols encoded /
 * decoded by those calls.  n >= 6. */
PC_API int pc_codec_host_stats(const pc_codec* c, double* out, int n);

/* Test aid: the conv epilogue evaluates GELU (layers/layers.py:45, nn.GELU) on two elements per lane with packed f32 instructions; this
 * compares that form with the contract's scalar pc_geluf (include/pc_math.h) over ALL 2^32 float arguments on the current device.
 * *n_mismatch must be 0; *n_nan_payload counts arguments for which both forms return NaN with different payload bits.  Synchronous. */
PC_API int pc_selftest_packed_gelu(uint64_t* n_mismatch, uint64_t* n_nan_payload);

/* Test aid: one launch of the conv launcher (every kernel, epilogue, operand and output form the codec uses) from a plain descriptor.
 * The launch parameters are built with the codec's own tap tables (conv k x k / transposed conv 5 s2 / the 192 -> 3 sub-pixel output layer)
 * and go through the same launcher as every codec layer.  Weights come from pc_pack_conv_weight with the same kind (kind 2: the sub-pixel
 * weights; its bias has 12 entries, bias[n] = b[n >> 2]).  Pointers are device pointers; asynchronous on `stream`.
 *   plan (optional, 2 ints): [0] the kernel instantiation the launcher chose (PC_PLAN_*), [1] the epilogue form (PC_FORM_*).
 * Returns PC_ERR_ARG for every launch the launcher refuses (nothing is written then). */
#define PC_TEST_MAX_SEG 8
typedef struct pc_test_conv_desc {
    /* input: nseg NHWC segments (channel axis = their concatenation), or smallc = 1: one input `seg_ptr[0]` of Cin channels, element
     * (b, y, x, c) at b * in_sb + y * in_sy + x * in_sx + c * in_sc */
    int nseg;
    const float* seg_ptr[PC_TEST_MAX_SEG];
    int seg_ld[PC_TEST_MAX_SEG];
    int seg_nch[PC_TEST_MAX_SEG];
    int smallc;
    int64_t in_sb, in_sy, in_sx, in_sc;
    int Cin, B, H, W;
    /* geometry: kind 0 conv k x k (padding k / 2) with `stride`, 1 ConvTranspose2d(5, s2, p2, op1), 2 the sub-pixel output layer */
    int kind, k, stride;
    int square;                            /* contract over x^2 (GDN / IGDN) */
    const float* w; const float* bias; int Cout;   /* Cout of the packed weights (kind 2: 12) */
    int epi;                               /* PC_EPI_* (progressivecodec_amd/csrc/pc_device.h) */
    const float* aux0; int ld0;
    const float* aux1; int ld1;
    const float* fg_gamma; const float* fg_beta;   /* fused input-layer GDN (3 -> 192) */
    float* out;
    int64_t out_sb, out_sy, out_sx, out_sc;
    int pixel_shuffle;
    float* out_relu;
    int ngroup;                            /* 2: a second GEMM on g1_seg0 / g1_w / g1_bias -> g1_out */
    const float* g1_seg0; const float* g1_w; const float* g1_bias; float* g1_out;
    int tile_cfg;                          /* PC_TILE_* of the layout-0 kernel (0: automatic) */
} pc_test_conv_desc;
#define PC_PLAN_UNI_16_3 1                 /* conv_igemm_uni_kernel<BK 16, 3 stages>: grids above 256 64x64 blocks */
#define PC_PLAN_UNI_32_2 2                 /* <BK 32, 2 stages>: small grids, K <= 256 per phase */
#define PC_PLAN_UNI_32_3 3                 /* <BK 32, 3 stages>: small grids */
#define PC_PLAN_UNI_32_2_SQ 4              /* <BK 32, 2 stages, x^2 operand>: GDN / IGDN */
#define PC_PLAN_UNI_OTHER 5                /* a tuning-only instantiation */
#define PC_PLAN_L0_64x64 6                 /* conv_igemm_kernel (weight layout 0) */
#define PC_PLAN_L0_64x64_SMALLC 7
#define PC_PLAN_L0_128x32 8
#define PC_PLAN_L0_128x32_SMALLC 9
#define PC_PLAN_L0_128x128 10
#define PC_PLAN_L0_128x128_SMALLC 11
#define PC_PLAN_IN_GDN 12                  /* conv_igemm_in_gdn_kernel */
#define PC_FORM_SLOW 1                     /* unified kernel: generic epilogue (any strides, aux read from global) */
#define PC_FORM_DIRECT 2                   /* unified kernel: dense output, rows in pixel order */
#define PC_FORM_TABLE 3                    /* unified kernel: LDS row table (permuted rows, strided output, PixelShuffle) */
#define PC_FORM_NCHW_PS 4                  /* unified kernel: NCHW PixelShuffle through LDS */
#define PC_FORM_L0_DIRECT 5                /* layout-0 kernel: dense output without aux tensors */
#define PC_FORM_L0_GENERIC 6               /* layout-0 kernel: generic epilogue */
#define PC_FORM_IN_GDN 7                   /* fused input-layer GDN */
PC_API int pc_test_conv(const pc_test_conv_desc* d, int* plan, void* stream);
/* pc_test_conv of a grouped launch (ngroup == 2) whose second GEMM reads an aux0 tensor of its own, g1_aux0, with the pixel stride ld0 of
 * the descriptor (the two branches' ResidualUnit tails of a window-attention module); NULL: pc_test_conv. */
PC_API int pc_test_conv_g1aux(const pc_test_conv_desc* d, const float* g1_aux0, int* plan, void* stream);

/* Test aid: one launch of a non-conv stage launcher (progressivecodec_amd/csrc/pc_stages.hip; GDN: the codec's own gdn()) from a plain
 * descriptor that carries the union of the launchers' arguments, the ones the wrappers above hide included (lik / lik_sb, mask_src /
 * mask_sb, yadd / ld_yadd, idx8, bias_ji, the quantile's batch stride and scratch, mu / ld_mu of the REM combine).  `size` must be
 * sizeof(pc_test_stage_desc): a mismatch returns PC_ERR_ARG before anything else is read.  Fields by kind:
 *   PREP_ENC / PREP_DEC_INDEX / PREP_DEQUANT   the pc_gc_prep_* arguments under their own names (B, HW; C must be 32)
 *   ATTENTION   x = qkv, aux0 = bias ([heads][T][T], bias_ji = 1: stored [h][j][i]), B H W C heads ws shift fscale, out
 *   GDN         x, aux0 = beta, aux1 = gamma [C_out][C_in], B H W C inverse, out
 *   QUANTILE    scale ld_scale B HW C q, out = thr [B], work (NULL: allocated by the launcher), sb (0: HW * ld_scale)
 *   EB_QUANT    x = z, aux0 = medians, B HW C, sym, out = zhat;   EB_DEQUANT  sym, aux0, out;   EB_LIK  sym, aux0, aux1 = net, out = lik
 *   REM         x = ret, ld_x, out = scale (updated in place), ld_scale, B HW, thr / mode_star, thr_bar / mode_bar, out2 = mu (or NULL), ld_mu
 *   NCHW_SLICE  x = src, sb = batch stride, B HW C, out
 *   SE          x, aux0 = fc1, aux1 = fc2, B HW C, out2 = part, out = s;   MAXPOOL  x, B H W C, out
 * plan (optional, 1 int): the kernel variant the launcher chose (PC_SPLAN_*), reported by the launcher itself.
 * Returns PC_ERR_ARG for every launch a launcher refuses (nothing is launched then).  Asynchronous on `stream`. */
typedef struct pc_test_stage_desc {
    int size;
    int kind;
    int B;
    int HW;
    int C;
    int H;
    int W;
    const float* scale;
    int ld_scale;
    const float* mu;
    int ld_mu;
    const float* y;
    int ld_y;
    const float* ybase;
    int ld_ybase;
    const float* yadd;
    int ld_yadd;
    const float* thr;
    int mask_mode;
    const float* mask_src;
    int64_t mask_sb;
    const float* table;
    int ntable;
    float bound;
    int32_t* sym;
    int32_t* idx;
    uint8_t* idx8;
    float* mask;
    float* yhat;
    int ld_yhat;
    float* lik;
    int64_t lik_sb;
    const float* x;
    int ld_x;
    const float* aux0;
    const float* aux1;
    float* out;
    float* out2;
    int heads;
    int ws;
    int shift;
    int bias_ji;
    float fscale;
    int inverse;
    float q;
    uint32_t* work;
    int64_t sb;
    const float* thr_bar;
    int mode_star;
    int mode_bar;
} pc_test_stage_desc;
enum { PC_STAGE_PREP_ENC = 1, PC_STAGE_PREP_DEC_INDEX = 2, PC_STAGE_PREP_DEQUANT = 3, PC_STAGE_ATTENTION = 4, PC_STAGE_GDN = 5,
       PC_STAGE_QUANTILE = 6, PC_STAGE_EB_QUANT = 7, PC_STAGE_EB_DEQUANT = 8, PC_STAGE_EB_LIK = 9, PC_STAGE_REM = 10,
       PC_STAGE_NCHW_SLICE = 11, PC_STAGE_SE = 12, PC_STAGE_MAXPOOL = 13 };
#define PC_SPLAN_SINGLE 1                  /* a launcher with one kernel (eb_*, rem_combine, nchw slice, SE squeeze, maxpool) */
#define PC_SPLAN_PREP_SCALAR 2             /* gc_prep_kernel / gc_dequant_kernel */
#define PC_SPLAN_PREP_VEC 3                /* gc_prep_vec_kernel<., false> / gc_dequant_vec_kernel */
#define PC_SPLAN_PREP_VEC_LIK 4            /* gc_prep_vec_kernel<0, true> */
#define PC_SPLAN_ATT_8_24 5                /* win_attention_kernel<8, 24> */
#define PC_SPLAN_ATT_4_80 6
#define PC_SPLAN_ATT_4_40 7
#define PC_SPLAN_Q_REG8 8                  /* quantile_thr_kernel<8>: n <= 8192 */
#define PC_SPLAN_Q_REG32 9                 /* quantile_thr_kernel<32>: n <= PC_QUANTILE_SMALL_N */
#define PC_SPLAN_Q_MULTI_VEC 10            /* sample -> bracket<true> -> final */
#define PC_SPLAN_Q_MULTI_SCALAR 11         /* sample -> bracket<false> -> final */
#define PC_SPLAN_GDN 16                    /* + the conv launcher's PC_PLAN_* of the GDN launch */
PC_API int pc_test_stage(const pc_test_stage_desc* d, int* plan, void* stream);

/* Debug/test taps: copy an internal device tensor of the last call to host ("y", "z", "latent_means", ...). */
PC_API int pc_codec_read_tap(pc_codec* c, const char* name, float* host_out, size_t cap_floats, size_t* n_floats);
PC_API int pc_codec_read_tap_i32(pc_codec* c, const char* name, int32_t* host_out, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif /* PCODEC_H */
