/*
 * filterbank.hip -- LDS-tiled, one-launch-per-level 2-D filter bank for gfx950.
 *
 * pywt.wavedec2 / waverec2 in periodization mode (ResNet/dwt_pruning.py:67-77) apply one
 * separable level at a time: analysis along axis -2 over the whole array, then along axis -1
 * (pywt/_multidim.py:183-191); synthesis along axis -1, then axis -2 (:288-309).  Each level
 * here is ONE kernel: a workgroup loads an input tile plus the filter halo into LDS once
 * (periodic / odd-length extension applied while loading), runs the first 1-D pass into LDS
 * and the second pass straight to HBM.  Every output sample is summed in PyWavelets' exact
 * order (csrc/wt_dwt_core.h: ascending taps in the interior, the split order at the right
 * edge, the special first synthesis site); only where the samples come from changes, so the
 * results are bit-identical to the two-pass kernels and to the oracle.  The two bands that
 * share a sample (lo/hi taps, or two subbands under one tap) are carried as a float2 so the
 * multiplies and adds issue as packed FP32 (v_pk_mul_f32 / v_pk_add_f32) -- still one
 * rounding per multiply and per add, as the contract requires (-ffp-contract=off).
 *
 * Forward tile: FR x FC outputs per subband; input tile (2 FR + F - 2) x (2 FC + F - 2).
 * Inverse tile: IR x IC outputs; coefficient tiles (IR/2 + F/2 + 1) x (IC/2 + F/2 + 1).
 *
 * One translation unit, in parts: the machine code of a tuned kernel depends on what shares its
 * unit (prune_unit.hip), so the parts are compiled together and the kernels' text is left alone.
 * fb_plan.h (tile geometry, LDS sizes, the interior rectangle, which kernel runs which tiles) also
 * compiles for the host alone: tests/test_fb_plan.py checks it without a GPU.
 */
#include "fb_device.inc"  /* what the kernels share: ana2*, syn_pass_*, extension indices */
#include "fb_fwd.inc"     /* FwdArgs, FwdGroup, k_fwd_level, k_fwd_int */
#include "fb_inv.inc"     /* InvArgs, InvGroup, k_inv_level, k_inv_int */
#include "fb_launch.inc"  /* items -> groups -> the plan's launches */
