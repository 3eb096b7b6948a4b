// kernels.hpp -- the __global__ kernels of libgypsum_hip.so (gfx950 only).
//
//   corr_cells_kernel   one workgroup per (stream, satellite, Doppler) cell, min(K, 8) wavefronts (K = samples per
//                       chip; K > 8 in rounds of 8 polyphase branches): per ms block carrier wipe-off + polyphase
//                       pre-sum (global -> LDS), then per wavefront FFT2048 -> x conj(PRN spectrum) -> IFFT2048 and
//                       |.| accumulation in registers (non-coherent), or the blocks folded before ONE transform
//                       (coherent); finally max / first-argmax / sum / count-of-max reductions.
//                       == utils.py:77-108 + the reductions of acquisition.py:180-189.
//   corr_cells_pipe_kernel  the same non-coherent cell for K == 8 (8.184 Msps, the acquisition search of the headline
//                       workload), software-pipelined: one workgroup per CU, 256 VGPRs, double-buffered rows in LDS,
//                       next block's samples prefetched during the transforms, replica spectrum resident in registers.
//   grid_fold_kernel / grid_cells[_wave]_kernel   flat grids whose satellites share the Doppler bins: wipe-off and
//                       pre-sum once per (stream, bin), then transform-only workgroups / wavefronts per satellite.
//   track_step_kernel   same core for one explicit millisecond of one tracking channel, plus the early/late taps
//                       and the rolled-PRN argmax of tracker.py:284-313.
//   track_block_kernel  persistent per-channel loop over many milliseconds with the DLL / Costas / lock-detector
//                       / circularity-watchdog state on the device (tracker.py:157-203, 246-262, 297-305, 331-389).
//                       One function, prologue / millisecond loop / epilogue (checkpoint copy, LDS carve, loop-state load
//                       and store are helpers beside it).  MODE 0: throughput form.  MODE 2 (K = 2, 8, 16; banks of at most one channel per CU): speculative
//                       form -- window correlations around the last peak lag on the serial chain, only the lock verdict
//                       between a peak and the next wipe-off, track_verify_kernel proving every such millisecond's
//                       arg-max from the full profile in parallel.
//   resample_kernel     rational-rate resampler (fs_in -> the stream format): file-width words widened and filtered by a
//                       polyphase FIR, one phase per lane, its taps in registers, the tile's input span in LDS.
//   iq_stats_kernel / iq_condition_kernel   signal conditioning: per-millisecond DC / power / peak / clipping records in a fixed
//                       float64 reduction order, and y = (x - dc) * gain in place behind whatever produced an ingest block.
//   iq_tones_kernel / iq_notch_kernel   narrowband interference: complex amplitudes of tones per block in a fixed float64 reduction
//                       order (spectrum scan, refinement), and their per-millisecond sequential projection out of the samples.
//   iq_blank_kernel / iq_power_hist_kernel   pulsed interference: per millisecond the hit bits of a power threshold through
//                       __ballot into LDS, dilated by the guard and applied (in place only the blanked samples are stored), and
//                       the eighth-octave histogram of the power the threshold is derived from, in integer atomics.
//   iq_excise_kernel / iq_spectrum_hist_kernel   narrowband and swept interference: per millisecond half-overlapped 256-point
//                       transforms, one wavefront per frame (radix 4, four points per lane, a 2 KiB LDS tile each); bins over a
//                       threshold and their guard are transformed back and subtracted (in place only corrected hops are stored),
//                       and the eighth-octave histogram of the bins' power the threshold is derived from, in integer atomics.
//   track_quality_kernel   signal quality: per (channel, window) sums of a block's tracking records -- peak moments, lock count,
//                       narrow/wide-band power ratios of 20-ms groups -- one wavefront each, in a fixed float64 reduction order.
//   hybrid_accumulate_kernel / hybrid_reduce_kernel   weak-signal acquisition: the power of a block's coherent profiles (corr_cells_kernel's)
//                       added at the code-Doppler-aligned lag into the row of the block's set, and per cell the arg-max, the second
//                       peak and the off-peak float64 moments of each set in a fixed order, the set with the larger z reported; the
//                       hybrid_*_cells / select / finish kernels are gyp_acquire_weak_dev's two-level bookkeeping.
//   weak_track_kernel   weak-signal tracking: one workgroup per channel of a weak bank; three code lags per sample against NCO replicas,
//                       a wavefront per millisecond in a fixed reduction order, bit synchronisation and the 20-ms PLL / DLL update
//                       in float64 on one lane between the periods (weak_plan.hpp holds that arithmetic for host and device).
//   weak_refine_* kernels   weak-signal hand-over: per candidate of the weak search the open-loop prompts a weak bank would write in
//                       SYNC, a wavefront per (candidate, millisecond) grid-wide, then one workgroup per candidate squares their
//                       pre-sums, scans a float64 periodogram for the residual Doppler and reports the bit edge and carrier phase
//                       (refine_plan.hpp holds that arithmetic for host and device).
//   weak_measure_* kernels   weak-signal measurement: per candidate of the hand-over and per pass the three-lag sums a weak bank would
//                       write and sum |x|^2 beside them, a wavefront per (candidate, millisecond) grid-wide, then one workgroup per
//                       candidate folds them over the data bits into early / prompt / late envelopes, corrects the code phase on the
//                       device for the next pass and reports it with the C/N0 (measure_plan.hpp holds that arithmetic for host and device).
//   acq_* kernels       the level-to-level bookkeeping of acquisition.py:70-152 on the device: plan, work list, record
//                       reuse (optional), float64 tie-breaks within a level (refine) and across levels (exact).
//
// The kernels live in the kernels_*.hpp parts below, one per family.
#pragma once
#include "kernels_common.hpp"
#include "kernels_cells.hpp"
#include "kernels_grid.hpp"
#include "kernels_track_step.hpp"
#include "kernels_track_block.hpp"
#include "kernels_dll_exact.hpp"
#include "kernels_bank.hpp"
#include "kernels_acq.hpp"
#include "kernels_misc.hpp"
#include "kernels_resample.hpp"
#include "kernels_level.hpp"
#include "kernels_notch.hpp"
#include "kernels_blank.hpp"
#include "kernels_excise.hpp"
#include "kernels_quality.hpp"
#include "kernels_hybrid.hpp"
#include "kernels_weak.hpp"
#include "kernels_refine.hpp"
#include "kernels_measure.hpp"
