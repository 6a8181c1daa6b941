/* pc_metrics.h -- C ABI of libpc_metrics.so: the evaluation metrics of the reference's harnesses (MS-SSIM and SSIM), on gfx950.
 *
 * Kept apart from libpcodec.so: the codec's numeric contract, byte strings and profiles do not depend on anything here.
 * Plain C, the conventions of pcodec.h: device pointers, int64 element strides, status codes PC_OK / PC_ERR_* (pcodec.h), `stream`
 * is a hipStream_t passed as void* (NULL = default stream).  No call allocates device memory or synchronises the host: the caller
 * passes a workspace, and every launch is ordered on `stream`.  Every argument is checked before the first HIP call.
 *
 * The metric is the public behaviour of pytorch_msssim 1.0 (ssim / ms_ssim), which the reference calls in
 * training/step.py:350-353 (via utils/functions.py:140, compute_msssim) and utils/eval_model/__main__.py:121; DESIGN.md section 9.
 */
#ifndef PC_METRICS_H
#define PC_METRICS_H

#include "pcodec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace pc_msssim needs for X, Y of shape [B, C, H, W], an odd window of win_size taps and `levels` scales;
 * 0 for arguments pc_msssim would reject as PC_ERR_ARG.  Layout: the per-block partial sums of every scale (f64 pairs), then the
 * 2x2-pooled X and Y of scales 1 .. levels-1 (each array 256-byte aligned). */
PC_API size_t pc_msssim_workspace_size(int B, int C, int H, int W, int win_size, int levels);

/* Replaces pytorch_msssim.ms_ssim(X, Y, data_range, size_average=False, win_size, win_sigma, weights, K) (levels >= 2;
 * training/step.py:350, utils/eval_model/__main__.py:121) and pytorch_msssim.ssim(X, Y, data_range, size_average=False, win_size,
 * win_sigma, K, nonnegative_ssim) (levels == 1; `weights` is then ignored and may be NULL).
 *   X, Y          float32 device tensors of logical shape [B, C, H, W]; element (b, c, h, w) at X[b*sxb + c*sxc + h*sxh + w] (all
 *                 strides > 0 and w contiguous: an unpadded view of a padded tensor needs no copy).
 *   win_size      odd, 1..31; win_sigma > 0: the Gaussian window, built here in float32 and normalised to sum 1.
 *   levels        1..5.  levels >= 2 requires min(H, W) > (win_size - 1) * 16 (the library's rule); levels == 1 requires H, W >= win_size.
 *   weights       host array of `levels` scale exponents (levels >= 2).
 *   nonnegative   levels == 1: relu on the per-channel SSIM (nonnegative_ssim=True).
 *   out           device float[B]: the value per image (the mean over its channels).
 *   out_scales    optional device double[levels][2][B][C]: per scale, the mean of the SSIM map ([s][0]) and of the CS map ([s][1]).
 * Per image, the result depends only on that image's planes: it is bitwise the same alone and inside any batch. */
PC_API int pc_msssim(const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb, int64_t syc, int64_t syh,
                     int B, int C, int H, int W, float data_range, int win_size, float win_sigma, float K1, float K2, int levels,
                     const float* weights, int nonnegative, void* workspace, size_t workspace_bytes, float* out, double* out_scales,
                     void* stream);

/* Host only, launches nothing: vec[s] for s < levels is 1 where a pc_msssim call with these arguments stages scale s with 16-byte loads
 * and 0 where it stages it float by float (both give the same bits).  Scale 0 reads X and Y: the 16-byte path needs both bases 16-byte
 * aligned and all six strides multiples of 4.  Scale s > 0 reads the pooled planes inside `workspace`: it needs a 16-byte aligned
 * workspace and W_s and H_s*W_s multiples of 4.  pc_msssim decides with the same code.  PC_ERR_ARG as pc_msssim. */
PC_API int pc_msssim_plan(const float* X, int64_t sxb, int64_t sxc, int64_t sxh, const float* Y, int64_t syb, int64_t syc, int64_t syh,
                          int B, int C, int H, int W, int win_size, int levels, const void* workspace, int* vec);

PC_API const char* pc_metrics_strerror(int code);
PC_API int pc_metrics_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PC_METRICS_H */
