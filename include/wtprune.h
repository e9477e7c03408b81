/*
 * wtprune.h -- C ABI of libwtprune.so, the MI355X (gfx950) implementation of the
 * DWT -> percentile-threshold -> IDWT weight-pruning path of iAmGiG/WaveletTransforms
 * (ResNet/dwt_pruning.py).  Plain pointers and sizes only; every device pointer is a HIP
 * device allocation owned by the caller; every entry point is stream-ordered on the given
 * hipStream_t (pass 0 for the null stream), never allocates, never synchronises, and is
 * safe to capture into a hipGraph.  Status: 0 = ok, < 0 = error (wtp_last_error() has the
 * message, phrased like the Python exception the reference would raise).
 *
 * Which reference interface each entry point replaces (file:line in /root/reference):
 *   wtp_wavelet_id / wtp_dec_len    pywt.Wavelet(name).dec_len        dwt_pruning.py:13
 *   wtp_max_level                   calculate_max_level               dwt_pruning.py:12-13
 *   wtp_prune_f32                   multi_resolution_analysis         dwt_pruning.py:35-95
 *                                   (per tensor of prune_layer_weights :98-127, which
 *                                    wavelet_pruning :130-174 calls per Conv2d)
 *   wtp_threshold_f32               percentile_based_thresholding     dwt_pruning.py:25-32
 *   wtp_wavedec2_f32                pywt.wavedec2 + coeffs_to_array   dwt_pruning.py:67-70
 *   wtp_waverec2_f32                array_to_coeffs + waverec2 + crop dwt_pruning.py:75-82
 *   wtp_prune_mode_f32              multi_resolution_analysis(mode=)  dwt_pruning.py:35, :67-68, :77
 *   wtp_prune_abs_f32               multi_resolution_analysis         dwt_pruning_NoEntropy.py:29-60
 *   wtp_prune_sweep_f32             multi_resolution_analysis at a grid of percentiles: the loop of
 *                                   main_pruning.py:186 over its thresholds, in one call
 *   wtp_prune_abs_sweep_f32         multi_resolution_analysis of dwt_pruning_NoEntropy.py:29-60 at a
 *                                   grid of absolute thresholds (the same loop), in one call
 *   wtp_prune_global_f32            (no reference counterpart: multi_resolution_analysis's transform and
 *                                   compare with ONE percentile threshold over all tensors' coefficients)
 *   wtp_prune_f16                   multi_resolution_analysis on float16 weights (model.half())
 *   wtp_synth_f32                   (test/bench input generator, no reference counterpart)
 */
#ifndef WTPRUNE_H
#define WTPRUNE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* wtp_stream_t; /* == hipStream_t */

#define WTP_MAX_DIMS 8
#define WTP_ABI_VERSION 1

/* error codes (mirroring the exception the reference path raises) */
#define WTP_OK 0
#define WTP_EBADWAVELET (-1) /* ValueError: Unknown wavelet name '...'                        */
#define WTP_EBADLEVEL (-2)   /* ValueError: Level value of L is too low . Minimum level is 0.  */
#define WTP_EBADPCT (-3)     /* ValueError: Percentiles must be in the range [0, 100]          */
#define WTP_EEMPTY (-4)      /* IndexError: percentile of an empty array                       */
#define WTP_ECROP (-5)       /* IndexError/RuntimeError: the 4-index crop at :79-82 fails      */
#define WTP_EARG (-6)        /* invalid argument (null pointer, too many dims, ...)           */
#define WTP_EWORKSPACE (-7)  /* workspace too small                                            */
#define WTP_EHIP (-8)        /* a HIP runtime call failed                                      */

typedef struct wtp_tensor {
    const float* in;                 /* device, contiguous C order                      */
    float* out;                      /* device, same shape; may alias `in` (in place)   */
    int32_t ndim;                    /* 0..8; >= 2 takes the wavelet path (:63-85)      */
    int32_t reserved;
    int64_t shape[WTP_MAX_DIMS];
} wtp_tensor;

/* Written by the device, one per tensor (copy back after the stream completes). */
typedef struct wtp_result {
    int64_t numel;          /* weights in the tensor                                 */
    int64_t zero_count;     /* (pruned == 0).sum()        dwt_pruning.py:88-89        */
    int64_t coeff_numel;    /* size of the packed coefficient array (percentile pop.)*/
    double thr64;           /* np.percentile(np.abs(coeff_arr), pct)      :27        */
    uint32_t thr32_bits;    /* float32(thr64): the compare of :31 runs in float32    */
    uint32_t max_abs_bits;  /* np.max(np.abs(coeff_arr)) as float32 bits  :29-30     */
    int32_t eff_level;      /* min(level, calculate_max_level(shape))     :64-65     */
    int32_t path;           /* selection: 1 window candidates, 2 window edges, 3 full scan,
                               4 the one-launch small path (exact three-digit radix select);
                               + 8 (9, 10, 11): the fused selection's patch window missed the ranks
                               and the segment was selected again over its coefficients;
                               5 a sweep's record; 6 a float16 tensor that got no transform (wtp_prune_f16);
                               7 a global percentile's record (wtp_prune_global_f32);
                               99 = the resident launch's grid was not co-resident (results invalid) */
} wtp_result;

/* ---- wavelets ---- */
int wtp_abi_version(void);
int wtp_wavelet_count(void);
const char* wtp_wavelet_name(int wavelet_id);
int wtp_wavelet_id(const char* name);           /* -1 if pywt would reject the name */
int wtp_dec_len(int wavelet_id);
int wtp_max_level(int64_t data_len, int dec_len); /* pywt.dwt_max_level */
int wtp_packed_shape(int64_t H, int64_t W, int level, int64_t* rows, int64_t* cols);

/* ---- the path: multi_resolution_analysis over a list of tensors ----
 * Semantics per tensor t, in order (exactly dwt_pruning.py:53-89):
 *   ndim < 2 : percentile_based_thresholding on the raw values (no wavelet check)
 *   ndim >= 2: level = min(level, max_level(min(H, W), dec_len)) -- the clamped level
 *              carries over to later tensors; wavedec2(periodization, axes (-2,-1));
 *              coeffs_to_array; threshold at the pct-th percentile of |coeffs| (NumPy 1.x
 *              linear interpolation, float32 compare); waverec2; crop; zero count.
 * Validation happens for all tensors before any device work; on error nothing is written.
 * Results: results_dev[t] (device memory).  Workspace: wtp_workspace_size bytes of device
 * memory (enough for wtp_prune_f32 and wtp_prune_layers_f32 of the same tensors; 0 if the
 * request itself is invalid), zeroed ONCE with wtp_workspace_init before first use; the library leaves it in
 * that state after every call (it is reusable by any later call with a workspace-size
 * request no larger than it). */
size_t wtp_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level);
int wtp_workspace_init(void* workspace, size_t bytes, wtp_stream_t stream);
int wtp_prune_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct,
                  void* workspace, size_t workspace_bytes, wtp_result* results_dev, wtp_stream_t stream);

/* wavelet_pruning / prune_layer_weights semantics (dwt_pruning.py:98-174): every tensor is an
 * independent call of multi_resolution_analysis([weight], ...), so the requested level is NOT
 * carried from one tensor to the next; otherwise identical to wtp_prune_f32 (one batched
 * launch sequence for all layers). */
int wtp_prune_layers_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct,
                         void* workspace, size_t workspace_bytes, wtp_result* results_dev, wtp_stream_t stream);

/* The general entry: flags = WTP_CARRY_LEVEL (wtp_prune_f32's level carry) | WTP_FLATTEN.
 * WTP_FLATTEN is the 1-D flattened mode (an extension: the reference's transform is 2-D): every
 * tensor with ndim >= 2 is transformed as ONE line, pywt.wavedec(w.ravel(), wavelet,
 * 'periodization', level) with the level clamped to pywt.dwt_max_level(numel, dec_len) (carried
 * over the list under WTP_CARRY_LEVEL), packed by pywt.coeffs_to_array ([cA_L | cD_L | ... |
 * cD_1]), thresholded at the pct-th percentile of |coeffs| exactly as the 2-D path, rebuilt by
 * pywt.waverec and cut to numel; ndim < 2 tensors keep the plain-percentile branch (:58-62).
 * WTP_NO_RESIDENT forces the three-launch form of level-0 groups for this call only (the retry of
 * tensors whose resident launch recorded WTP_PATH_FAULT).
 * Workspace: wtp_workspace_size_ex with the same flags. */
#define WTP_CARRY_LEVEL 1
#define WTP_FLATTEN 2
#define WTP_NO_RESIDENT 4
size_t wtp_workspace_size_ex(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags);
int wtp_prune_ex_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                     void* workspace, size_t workspace_bytes, wtp_result* results_dev, wtp_stream_t stream);

/* ---- PyWavelets' signal-extension modes: the `mode` argument of multi_resolution_analysis
 * (dwt_pruning.py:35), handed to pywt.wavedec2 / waverec2 (:67-68, :77) ----
 * wtp_prune_mode_f32 is wtp_prune_ex_f32 with a mode: WTP_MODE_PERIODIZATION is that entry
 * itself; zero, constant, symmetric, reflect and periodic run the same path with the mode's
 * geometry, bit for bit as PyWavelets 1.1.1 computes it in float32:
 *   - a level turns a side N into floor((N + F - 1) / 2) coefficients (not ceil(N / 2)), so the
 *     packed array of coeffs_to_array is larger than the tensor and in general not tight; its
 *     padding zeros belong to the percentile's population (coeff_numel counts them);
 *   - a level's synthesis gives 2N - F + 2 samples; waverec2 drops one between levels where that
 *     is one more than the next level's detail bands hold;
 *   - the result (2 R1 - F + 2, 2 C1 - F + 2) is H + (H odd) by W + (W odd): a 4-D tensor is
 *     cropped by :79-82, a 2-D or 3-D tensor with an odd side is WTP_ECROP (an odd Linear weight
 *     included), as under periodization.
 * The level clamp (pywt.dwt_max_level) does not depend on the mode, and a tensor whose clamped
 * level is 0, or with ndim < 2, takes exactly the periodization path (byte-identical results).
 * smooth, antisymmetric and antireflect have ids but are not implemented (WTP_EARG), WTP_FLATTEN
 * with any mode but periodization is WTP_EARG, and so is a wavelet of odd filter length under an
 * extension mode.  Tensors whose images are at most 8 x 8 run their whole forward transform in
 * one launch and their whole inverse transform in another, each image held on chip in between
 * its read and its write; larger ones run a level at a time.  Same rules as every entry: stream-
 * ordered, no allocation, no synchronisation, capturable, out may alias in, validation before any
 * device work.  Workspace: wtp_workspace_size_mode bytes (0 if the request is invalid), shared with
 * and initialised like wtp_prune_f32's. */
#define WTP_MODE_PERIODIZATION 0
#define WTP_MODE_ZERO 1
#define WTP_MODE_CONSTANT 2
#define WTP_MODE_SYMMETRIC 3
#define WTP_MODE_REFLECT 4
#define WTP_MODE_PERIODIC 5
#define WTP_MODE_SMOOTH 6        /* known to pywt, not implemented here */
#define WTP_MODE_ANTISYMMETRIC 7 /* " */
#define WTP_MODE_ANTIREFLECT 8   /* " */
int wtp_mode_id(const char* name);       /* -1 if pywt would reject the name */
const char* wtp_mode_name(int mode_id);  /* NULL for an unknown id */
/* pywt.coeffs_to_array's shape for an H x W image (the level is taken as given, not clamped) */
int wtp_packed_shape_mode(int64_t H, int64_t W, int wavelet_id, int level, int mode_id, int64_t* rows, int64_t* cols);
size_t wtp_workspace_size_mode(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags,
                               int mode_id);
int wtp_prune_mode_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                       int mode_id, void* workspace, size_t workspace_bytes, wtp_result* results_dev,
                       wtp_stream_t stream);
/* components, as wtp_wavedec2_f32 / wtp_waverec2_f32 below (level as given; packed: (B, rows,
 * cols) of wtp_packed_shape_mode, padding zeroed; waverec2 crops to H x W) */
size_t wtp_dwt_workspace_size_mode(int64_t B, int64_t H, int64_t W, int wavelet_id, int level, int mode_id);
int wtp_wavedec2_mode_f32(const float* in, float* packed, int64_t B, int64_t H, int64_t W, int wavelet_id,
                          int level, int mode_id, void* workspace, size_t workspace_bytes, wtp_stream_t stream);
int wtp_waverec2_mode_f32(const float* packed, float* out, int64_t B, int64_t H, int64_t W, int wavelet_id,
                          int level, int mode_id, const float* thr32_dev, void* workspace, size_t workspace_bytes,
                          wtp_stream_t stream);

/* ---- the absolute-threshold method: multi_resolution_analysis of
 * ResNet/dwt_pruning_NoEntropy.py:29-60 over a list of tensors ----
 * Semantics per tensor, in order:
 *   ndim < 2 : out = where(|w| < thr32, +0, w); the wavelet is not looked up
 *   ndim >= 2: wavedec2(periodization, axes (-2,-1)) at the REQUESTED level (no clamp, no carry:
 *              PyWavelets only warns above dwt_max_level, and lines shorter than the filter wrap
 *              more than once); coeffs_to_array (zero padding where the packing is not tight);
 *              every packed cell with |c| < thr32 becomes +0; waverec2; every axis cropped to
 *              the original shape (a generic slice: odd 2-D tensors are valid, no WTP_ECROP).
 * thr32 is the threshold rounded to the nearest float32 (NumPy 1.x compares a float32 array
 * with a Python float in float32; overflow gives +inf): NaN, zero and negative thresholds
 * prune nothing, +inf prunes every finite coefficient.
 * Validation before any device work: unknown wavelet for an ndim >= 2 tensor WTP_EBADWAVELET,
 * level < 0 WTP_EBADLEVEL, level > 32 WTP_EARG, an empty ndim >= 2 tensor WTP_EARG; an empty
 * 1-D tensor is a no-op with a zeroed record.
 * Tensors whose images are at most 8 x 8 all run in one launch that keeps each image on chip
 * between its read and its write (path 1; groups of 64 tensors); larger ones run the filter-bank
 * chain through a packed array in the workspace (path 2); ndim < 2 and level 0 of larger
 * tensors are a plain mask (path 0).  Workspace: wtp_abs_workspace_size bytes (0 if the request
 * is invalid); it needs no initialisation and a call of tiny tensors only needs the same few
 * bytes whatever its batch.  It is plain scratch, written from its first byte and left as it
 * is: it MUST NOT be the workspace of wtp_prune*_f32 / wtp_threshold_f32 / wtp_min_prune_f32,
 * whose selection and barrier state at the start of that workspace has to stay as those
 * entries leave it (a buffer that held an abs call needs wtp_workspace_init before they use it).  Stream-ordered, no allocation, no synchronisation, capturable;
 * out may alias in. */
typedef struct wtp_abs_result {   /* one per tensor, device memory */
    int64_t numel;
    int64_t nonzero_in;    /* torch.count_nonzero(weight): -0.0 is zero, NaN is non-zero */
    int64_t nonzero_out;   /* torch.count_nonzero(pruned)                                */
    int64_t coeff_numel;   /* packed coefficient array size (numel for ndim < 2)         */
    uint32_t thr32_bits;   /* float32(threshold), the value the compare used             */
    int32_t level;         /* the level that ran (the requested one; 0 for ndim < 2)     */
    int32_t path;          /* 1 = fused tiny-image launch, 2 = filter-bank chain, 0 = plain mask */
    int32_t reserved;
} wtp_abs_result;
#define WTP_ABS_PATH_MASK 0
#define WTP_ABS_PATH_TINY 1
#define WTP_ABS_PATH_CHAIN 2
size_t wtp_abs_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level);
int wtp_prune_abs_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double threshold,
                      void* workspace, size_t workspace_bytes, wtp_abs_result* results_dev, wtp_stream_t stream);

/* ---- the absolute-threshold sweep: one call prunes the list at up to eight absolute thresholds
 * (the threshold grid of ResNet/main_pruning.py under dwt_pruning_NoEntropy.py's method) ----
 * For every k < nthr the outputs outs[k * ntensors + t] and the records
 * results_dev[k * ntensors + t] (threshold-major: block k of the records is laid out like the
 * records of one ordinary call) are, bit for bit and field for field (path included), what
 * wtp_prune_abs_f32(tensors, ..., thresholds[k], ...) gives: the unclamped level, the float32
 * rounding of the threshold (NaN, zero and negative thresholds prune nothing, +inf and 1e40 prune
 * every finite coefficient), the generic crop, both non-zero counts (nonzero_in is counted on the
 * input before any output is written), and the same choice among the three paths.  The method
 * selects nothing, so a tensor is read and transformed forward ONCE and every threshold costs
 * one mask and inverse: tiny-image tensors (path 1) keep their raw coefficients on chip and run
 * every threshold's inverse over them in the same launch (groups of 24 tensors); a chain tensor
 * (path 2) keeps one packed array in the workspace, read with threshold k on the load by the k-th
 * inverse; a plain mask (path 0) is one masked copy per threshold.
 * thresholds (host memory) may repeat and need not be sorted: every k is answered on its own.
 * tensors[t].out is ignored and may be NULL.  AT MOST ONE output of a tensor may be the tensor's
 * input (in place); the other outputs must not overlap it.
 * Validation before any device work, nothing written on error: everything wtp_prune_abs_f32
 * rejects, nthr outside [1, WTP_ABS_SWEEP_MAX_THR] or thresholds == NULL (WTP_EARG), a NULL
 * output of a non-empty tensor (WTP_EARG), two outputs of one tensor at the same address
 * (WTP_EARG).
 * Workspace: wtp_abs_sweep_workspace_size bytes (0 if the request is invalid), the rules of
 * wtp_prune_abs_f32's: no initialisation, plain scratch of this entry, NOT the workspace of the
 * percentile entries; a call of tiny tensors only needs the same few bytes whatever its batch and
 * nthr.  Stream-ordered, no allocation, no synchronisation, capturable. */
#define WTP_ABS_SWEEP_MAX_THR 8
size_t wtp_abs_sweep_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int nthr);
int wtp_prune_abs_sweep_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level,
                            const double* thresholds /* host */, int nthr,
                            float* const* outs /* host array of nthr * ntensors device pointers */, void* workspace,
                            size_t workspace_bytes, wtp_abs_result* results_dev /* nthr * ntensors */,
                            wtp_stream_t stream);

/* ---- the percentile sweep: one call prunes the list at several percentiles (the experiment of
 * ResNet/main_pruning.py:186, the same model and wavelet at a grid of thresholds) ----
 * For every k < npct the outputs outs[k * ntensors + t] and the records results_dev[k * ntensors + t]
 * (percentile-major: block k of the records is laid out like the records of one ordinary call)
 * are, bit for bit and field for field, what wtp_prune_ex_f32(tensors, ..., pcts[k],
 * flags & WTP_CARRY_LEVEL, ...) gives under periodization, except that path reads WTP_PATH_SWEEP:
 * the level clamp and its carry, the ndim < 2 branch, padding zeros of a packed array that is not
 * tight, NumPy 1.x's lerp, the float32 compare, the NaN rule, the crops and their WTP_ECROP cases.
 * The forward transform runs once, one exact selection finds the order statistics of all the
 * percentiles (three histogram passes over the population whatever npct is; tie-heavy populations
 * cost the same), then every percentile's mask or inverse transform writes its output.
 * tensors[t].out is ignored and may be NULL.  pcts (host memory) may hold duplicates and need
 * not be sorted: every k is answered on its own.
 * flags: WTP_CARRY_LEVEL as elsewhere; WTP_SWEEP_THRESHOLDS_ONLY stops after the selection: the
 * records carry every field with zero_count = 0, outs may be NULL and no output is written.
 * WTP_FLATTEN, WTP_NO_RESIDENT and any other bit are WTP_EARG; periodization only.
 * Validation before any device work, nothing written on error: everything wtp_prune_ex_f32
 * rejects, and npct outside [1, WTP_SWEEP_MAX_PCT] or pcts == NULL (WTP_EARG), a pcts[k] outside
 * [0, 100] or NaN (WTP_EBADPCT), a NULL output pointer without WTP_SWEEP_THRESHOLDS_ONLY
 * (WTP_EARG), two outputs of one tensor at the same address (WTP_EARG).  AT MOST ONE output of a
 * tensor may be the tensor's input (in place); the other outputs must not overlap it.
 * Workspace: wtp_sweep_workspace_size bytes (0 if the request is invalid).  It needs no
 * initialisation (the call's first kernel zeroes what it accumulates into) and is plain scratch
 * of this entry alone: like the absolute-threshold workspace it MUST NOT be the workspace of
 * wtp_prune*_f32 / wtp_threshold_f32 / wtp_min_prune_f32.  Stream-ordered on the caller's stream
 * only, no allocation, no synchronisation, capturable. */
#define WTP_SWEEP_MAX_PCT 8
#define WTP_SWEEP_THRESHOLDS_ONLY 16 /* a flag of this entry only */
#define WTP_PATH_SWEEP 5
size_t wtp_sweep_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int npct,
                                int flags);
int wtp_prune_sweep_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level,
                        const double* pcts /* host */, int npct, int flags,
                        float* const* outs /* host array of npct * ntensors device pointers */, void* workspace,
                        size_t workspace_bytes, wtp_result* results_dev /* npct * ntensors */, wtp_stream_t stream);

/* ---- the global percentile: one threshold over the whole list (global magnitude pruning in the
 * wavelet domain; an addition, the reference prunes per tensor) ----
 * The level clamp, its carry (flags & WTP_CARRY_LEVEL) and the ndim < 2 branch are those of the
 * sweep.  A tensor that gets a transform (ndim >= 2 and a clamped level >= 1) contributes its whole
 * packed coefficient array, coeffs_to_array(wavedec2(...)) under periodization with the padding
 * zeros of a packing that is not tight, exactly its population in the per-tensor entries; every
 * other tensor contributes its raw values.  The POOL is the concatenation, N keys |x|.  For every
 * k < npct: thr64 is NumPy 1.x's linear percentile pcts[k] of the pool (the two order statistics
 * of rank (N - 1) pcts[k] / 100, their difference in float32, the blend in float64, from the upper
 * end when gamma >= 0.5, NaN if the pool holds a NaN), thr32 = float32(thr64), and every tensor's
 * output outs[k * ntensors + t] is where(|c| < thr32, +0, c) in float32, through waverec2 and its
 * crop for a transformed tensor.  The per-tensor entries and this one share everything but the
 * population: the forward transform runs once, one exact selection (three histogram passes over
 * the pool whatever npct is, one shared state and one set of histograms for every tensor) finds
 * all order statistics, every percentile's mask or inverse reads the pool's threshold.
 * Records results_dev[k * ntensors + t] (percentile-major, as the sweep's): numel, coeff_numel,
 * eff_level and zero_count are tensor t's own; thr64, thr32_bits and max_abs_bits are the pool's,
 * the same in every record of percentile k (the maximum is the pool's because the thresholded
 * array is the pool); path = WTP_PATH_GLOBAL.
 * Arguments, flags (WTP_CARRY_LEVEL, WTP_SWEEP_THRESHOLDS_ONLY; any other bit is WTP_EARG), the
 * output layout, the in-place rule (at most one output of a tensor may be its input), validation
 * order and error codes are wtp_prune_sweep_f32's, and one more: a pool of more than 2^32 - 1 keys
 * is WTP_EARG with a message naming the count (ranks, residuals and bins are 32 bits wide, and one
 * bin may hold the whole pool).
 * An empty pool is answered as the sweep answers the same list: ntensors == 0 is WTP_OK with nothing
 * written (after the percentile check: a bad percentile is WTP_EBADPCT even then), and a list
 * with an empty tensor is WTP_EEMPTY at that tensor -- the reference's percentile of an empty
 * array -- so a call that reaches the device never has an empty pool.
 * Workspace: wtp_global_workspace_size bytes (0 if the request is invalid, an over-full pool
 * included).  Like the sweep's it needs no initialisation and is plain scratch of this entry
 * alone: it MUST NOT be the workspace of wtp_prune*_f32 / wtp_threshold_f32 / wtp_min_prune_f32.
 * Stream-ordered on the caller's stream only, no allocation, no copy from host memory, no
 * synchronisation, capturable. */
#define WTP_PATH_GLOBAL 7
size_t wtp_global_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int npct,
                                 int flags);
int wtp_prune_global_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level,
                         const double* pcts /* host */, int npct, int flags,
                         float* const* outs /* host array of npct * ntensors device pointers */, void* workspace,
                         size_t workspace_bytes, wtp_result* results_dev /* npct * ntensors */, wtp_stream_t stream);

/* ---- float16 weights: multi_resolution_analysis on the tensors of model.half() ----
 * The reference takes float16 weights as they come (dwt_pruning.py:56 .numpy(), :61 / :84 rebuild
 * with dtype=weight.dtype); wtp_prune_f16 is wtp_prune_mode_f32 for them.  The descriptor is the
 * same wtp_tensor, but its `in` / `out` are read and written as IEEE binary16 words (numel of
 * them, 2-byte aligned; cast the pointers).  Per tensor, what NumPy 1.x and PyWavelets 1.1.1 do:
 *   a tensor that gets a transform (ndim >= 2 and a clamped level >= 1, in any mode): wavedec2
 *     widens to float32, so it runs exactly as wtp_prune_mode_f32 on float32(w) and the float32
 *     result is narrowed once, round to nearest even; its record is that call's, with zero_count
 *     counted AFTER the narrowing (a float32 result of at most 2^-25 in magnitude is a zero);
 *   a tensor that gets none (ndim < 2, or level 0 after the clamp): everything stays float16.
 *     thr64 is np.percentile of the float16 array -- the two order statistics' difference is
 *     NumPy's half subtraction (the float32 difference rounded to half), the blend runs in
 *     float64 -- and the compare |w| < thr runs in float16 on half(thr64) (one rounding from
 *     float64): thr32_bits holds that value widened to float32, max_abs_bits the widened float16
 *     maximum, coeff_numel = numel, path = WTP_PATH_HALF.  Pruned words are +0, the others keep
 *     their bits.  The selection is exact by construction: |w| has 2^15 possible keys, found by
 *     two histogram passes (11 + 4 bits); no sample, no window, no other path.
 * Not covered: inputs with |w| >= 65000, +-inf or NaN (NumPy changes the compare's type there, or
 * the threshold is NaN).  They are safe to pass, but no parity with the reference is claimed.
 * flags: WTP_CARRY_LEVEL as elsewhere; WTP_NO_RESIDENT is accepted and ignored (no float16 tensor
 * reaches the resident launch); WTP_FLATTEN is WTP_EARG (the flattened mode is float32 only).
 * Everything else as wtp_prune_mode_f32: validation of every tensor in the reference's order before
 * any device work (a tensor of more than 2^31-1 weights is WTP_EARG: the histogram counts are 32
 * bits wide), no allocation, no synchronisation, capturable, out may alias in.
 * Workspace: wtp_workspace_size_f16 bytes (0 if the request is invalid), zeroed once with
 * wtp_workspace_init and this entry's own: it begins with the float32 call's workspace for the
 * transformed tensors, kept as that call keeps it, followed by scratch that every call zeroes
 * itself (do not hand it to a float32 entry). */
#define WTP_PATH_HALF 6
size_t wtp_workspace_size_f16(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags,
                              int mode_id);
int wtp_prune_f16(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                  int mode_id, void* workspace, size_t workspace_bytes, wtp_result* results_dev, wtp_stream_t stream);

/* percentile_based_thresholding(arr, pct) on n device floats: out = where(|in| < thr, 0, in) */
int wtp_threshold_f32(const float* in, float* out, int64_t n, double pct, void* workspace,
                      size_t workspace_bytes, wtp_result* result_dev, wtp_stream_t stream);

/* components: batch of B images of H x W (row-major), packed coefficient array (B, rows, cols)
 * as wtp_packed_shape; waverec2 optionally thresholds every coefficient on load with the
 * float32 threshold read from thr32_dev (device pointer; NULL = no threshold) and crops to H x W. */
size_t wtp_dwt_workspace_size(int64_t B, int64_t H, int64_t W, int level);
int wtp_wavedec2_f32(const float* in, float* packed, int64_t B, int64_t H, int64_t W, int wavelet_id,
                     int level, void* workspace, size_t workspace_bytes, wtp_stream_t stream);
int wtp_waverec2_f32(const float* packed, float* out, int64_t B, int64_t H, int64_t W, int wavelet_id,
                     int level, const float* thr32_dev, void* workspace, size_t workspace_bytes,
                     wtp_stream_t stream);

/* synthetic inputs (csrc/wt_synth.h): out[k] = wt_synth_value(seed, tensor_id, k, e) */
int wtp_synth_f32(float* out, int64_t n, uint64_t seed, uint32_t tensor_id, int e, wtp_stream_t stream);

/* percentage_min_pruning (ResNet/min_weight_pruning.py:66-74) for a batch of tensors (the
 * min_weight_pruning baseline of :77-139): in every tensor zero the k = int(numel * fraction)
 * entries of smallest |w| (flattened).  Among entries with |w| equal to the k-th smallest the
 * lowest flat indices are pruned first (torch.topk leaves that order unspecified; counts are
 * exact either way).  k outside [0, numel] is WTP_EARG ("selected index k out of range").
 * out may alias in.  Results: numel, zero_count (zeros of out), thr64/thr32_bits = the k-th
 * smallest |w| (0 when k = 0).  Workspace: wtp_min_prune_workspace_size bytes, zeroed once
 * with wtp_workspace_init. */
size_t wtp_min_prune_workspace_size(const wtp_tensor* tensors, int ntensors, double fraction);
int wtp_min_prune_f32(const wtp_tensor* tensors, int ntensors, double fraction, void* workspace,
                      size_t workspace_bytes, wtp_result* results_dev, wtp_stream_t stream);

/* random_pruning (ResNet/random_pruning.py:49-56) for a batch of tensors: in tensor t zero
 * prune_counts[t] (host array; torch.randperm(numel)[:k] slicing: k > numel takes all, k < 0
 * takes numel + k) distinct flat positions drawn by a keyed pseudo-random permutation of
 * [0, numel) (csrc/wt_perm.h; seed + tensor index).  torch's Philox stream is not reproduced:
 * the positions differ from the reference's, the counts follow the same rule.  out may alias
 * in.  Results: numel and zero_count (zeros of out, NaN counted as non-zero). */
int wtp_random_prune_f32(const wtp_tensor* tensors, int ntensors, const int64_t* prune_counts, uint64_t seed,
                         wtp_result* results_dev, wtp_stream_t stream);

/* calculate_sparsity's count (testing_suite/eval_model.py:7-20): *count_dev = #(|x| < thr) over n
 * device floats (NaN is not counted). */
int wtp_count_small_f32(const float* x, int64_t n, float thr, unsigned long long* count_dev, wtp_stream_t stream);

/* measurement hook (bench.py): hipEvent_t handles recorded on the call's stream at the stage
 * boundaries of later wtp_prune*_f32 calls on this thread -- [0] start, [1] forward DWT done,
 * [2] k_window, [3] k_collect, [4] k_mask_select, [5] inverse DWT done (first segment group).
 * n = 0 disables. */
int wtp_set_stage_events(void* const* events, int n);

/* Level-0 launch groups whose chunks fit the device's co-resident grid (wtp_resident_capacity
 * workgroups of 49152 weights, one per CU) run as ONE launch that keeps every weight in
 * registers between its read and its masked write (k_resident).  It needs the CUs to itself
 * while it runs; mode 0 always uses the three-launch form (window / collect / mask-select).
 * Returns the previous mode (process-wide). */
int wtp_set_resident(int mode);
int wtp_resident_capacity(void); /* 0 if the current device cannot host the resident launch */
/* Bound (microseconds) of every wait inside the resident launch; returns the previous bound.  A
 * launch whose workgroups were not all resident at once times out there and stores NOTHING for
 * the tensors concerned (inputs untouched; outputs untouched too, except as wtp_set_resident_early
 * says for out-of-place tensors): their records read path == 99
 * (WTP_PATH_FAULT), and the caller re-runs exactly those tensors with wtp_set_resident(0).
 * Default 2000 (about 75x a full ResNet-18 resident launch), at most 40000000 (larger values are clamped: the bound is kept in 32-bit
 * ticks of the 100 MHz wall clock); tests lower it to force the fault path. */
unsigned wtp_set_resident_timeout_us(unsigned us);
#define WTP_PATH_FAULT 99
/* Early stores of the resident launch.  A tensor of more than one workgroup (49152 weights) has
 * its percentile selected by a workgroup of its own; as soon as that selector knows the key range
 * [lo, hi] holding the threshold (1/1024 of the sample window) it publishes it, and the tensor's
 * workgroups store at once every 64-lane float4 store none of whose weights has |w| in [lo, hi]
 * (|w| < lo: 0, |w| > hi: kept -- exact, not speculative); the few per cent left wait for the
 * threshold.  Identical results.  Out of place only: a tensor pruned in place keeps "all of it
 * stored or none".  Out of place, a tensor whose wait times out AFTER its range was published
 * may be left with its OUTPUT partly written (its input is never touched): its record still reads
 * path == 99 and the re-run overwrites the whole output.  Mode 1 (default) on, 0 off, 2 on with
 * the stores counted (measurement: two atomic adds per wave); any other value is rejected
 * (WTP_EARG).  Returns the previous mode (process-wide).  The environment variable
 * WTP_RESIDENT_EARLY (0 / 1 / 2) sets the mode a process starts with. */
int wtp_set_resident_early(int mode);
/* Mode 2's counters of `workspace` (the one passed to the prune calls): wave-wide float4 stores
 * issued on the range / held back for the threshold since the last read; waits for `stream`,
 * reads them and clears them. */
int wtp_resident_early_counts(void* workspace, wtp_stream_t stream, unsigned long long* early,
                              unsigned long long* deferred);
/* A call with more than one launch group (24 tensors) of wavelet-transformed tensors runs each
 * group's percentile selection on a side stream of the library's (one per device and caller
 * stream, non-blocking, created on first use), overlapping the next group's forward transform;
 * the caller's stream waits for it before that group's inverse, so the call stays ordered on
 * the caller's stream (graph capture included).  Mode 0: everything on the caller's stream; any
 * other value is rejected (WTP_EARG).  Returns the previous mode (process-wide). */
int wtp_set_pipeline(int mode);
/* Fused selection for launch groups of large wavelet-transformed tensors (each >= 2^22 packed
 * coefficients, every forward level in the tiled interior kernels, at most 6 levels, images of at
 * least 128 x 128): the percentile window comes from a transform of four 128 x 128 input patches
 * before the forward, the forward classifies the coefficients as it writes them, and the packed
 * array is not read again for the selection (identical results: a window that misses the ranks is
 * caught by the select, which then takes its exact full scan).  Mode 1 (default) on, 0 off; any
 * other value is rejected (WTP_EARG).  Returns the previous mode (process-wide). */
int wtp_set_fused_select(int mode);
/* The filter-bank levels run their interior tiles (input window inside the image, full tile)
 * in kernels compiled without the edge forms and the frame of edge tiles in the same kernels'
 * edge-capable form (mode 2); mode 3 (default) as 2, but a small level (a few thousand tiles)
 * runs every tile in one launch of the edge-capable form; mode 1: the frame in the general
 * kernel; mode 0: every tile in the general kernel (identical results in every mode).  Returns the
 * previous mode (process-wide). */
int wtp_set_interior(int mode);
#define WTP_PATH_SMALL 4 /* every tensor of the call ran in one launch (2-D transforms, small population) */
/* measurement hook (bench.py): while set, every resident launch atomically lowers stamps_dev[0] to
 * its first workgroup's start and raises stamps_dev[1] to its last workgroup's end (after that
 * workgroup's stores completed), in ticks of the 100 MHz wall clock -- the launch's span on the
 * device, free of the host's dispatch gaps.  The caller initialises [0] = ~0, [1] = 0; NULL = off. */
int wtp_set_kernel_stamps(unsigned long long* stamps_dev);

const char* wtp_last_error(void);
int wtp_last_error_tensor(void); /* index of the tensor that failed validation, or -1 */

#ifdef __cplusplus
}
#endif
#endif
