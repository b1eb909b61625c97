// sdft_kernels.hpp -- the hand-written HIP kernels for gfx950 (CDNA4) of the modulated Sliding DFT hot path, by stage.
// Citations in the stage files are into /root/reference/c/src/sdft/sdft.h.
//
//   sdft_base.hpp          complex helpers, cross-lane (DPP) neighbour fetch, K0 delta_kernel (differences + delay line),
//                          the recurrence step (sdft.h:572-585), the completion word of short synchronous calls
//   sdft_carry_fast.hpp    K1a/K1b  carries of the chunk-parallel FD double path: chunk_sum_kernel, chunk_fft_kernel,
//                          chunk_fft_mixed_kernel (partial sums per chunk), carry_scan_kernel (scan over chunks)
//   sdft_carry_exact.hpp   K1a'  the reference's rounding sequence (FD float always): carry_exact_kernel (serial pass),
//                          fid_seed_kernel + carry_relay_kernel (one dependent addition per step on the chain)
//   sdft_forward.hpp       K1    window (sdft.h:350-402), ForwardArgs, flow-mode waits, self-carried chunks (fold + FFT in
//                          LDS), forward_kernel (independent waves with halo lanes: any N, row-pointer outputs)
//   sdft_forward_every.hpp K1e   forward_every_kernel: forward_kernel's tiles, acc and fid stepped for every sample, only the
//                          rows of a call-local grid (every-th sample) demodulated, windowed and stored (sdft_hip_sdft_every_n)
//   sdft_forward_power.hpp K1p   forward_power_kernel: forward_every_kernel's grid plus a band of bins, re^2 + im^2 of the windowed
//                          bin formed in registers and stored as one real number (sdft_hip_sdft_power_n)
//   sdft_forward_power_sum.hpp K1s forward_pooled_power_kernel: that power at every sample, summed in registers over the windows of the
//                          grid, one store per window; pooled_power_rows_kernel adds the pieces of the windows a chunk boundary cuts
//                          (sdft_hip_sdft_power_sum_n)
//   sdft_forward_power_peak.hpp K1k forward_power_peak_kernel: the pooled power kernel with the other statistic -- the largest or the
//                          smallest of those powers over each window, kept in registers by one rule (peak_hold); peak_rows_kernel
//                          combines the pieces of the windows a chunk boundary cuts (sdft_hip_sdft_power_peak_n)
//   sdft_forward_power_smooth.hpp K1o forward_power_smooth_kernel: the pooled power kernel with a recursion for the sum -- the one-pole
//                          average s = a s + b p of those powers, advanced at every sample, stored on the grid and never cleared;
//                          smooth_scan_kernel carries it across the time chunks in ascending order, smooth_fix_kernel adds what the
//                          later chunks left out of their rows (sdft_hip_sdft_power_smooth_n)
//   sdft_forward_cross_sum.hpp K1x forward_cross_sum_kernel: the pooled power kernel with a second channel -- A conj(B) of the windowed
//                          bins of two channels of a plan, summed in registers over the windows of the grid (sdft_hip_sdft_cross_sum_n)
//   sdft_forward_cross_smooth.hpp K1xs forward_cross_smooth_kernel: the cross-spectrum kernel with the smoothed power kernel's recursion
//                          for the sums -- the one-pole average of A conj(B) per component, advanced at every sample and stored on the
//                          grid; smooth_scan_kernel and smooth_fix_kernel carry it across the time chunks as 2 * nbins real numbers
//                          per pair (sdft_hip_sdft_cross_smooth_n)
//   sdft_forward_smooth_peak.hpp K1os forward_smooth_peak_kernel: the peak-hold kernel with the smoothed power kernel's recursion in the
//                          loop -- the largest or the smallest of the one-pole average over each window; every chunk starts from the
//                          value smooth_scan_kernel left for it after a carry pass of forward_power_smooth_kernel, peak_rows_kernel
//                          combines the pieces of the windows a chunk boundary cuts (sdft_hip_sdft_smooth_peak_n)
//   sdft_forward_lag_sum.hpp K1l forward_lag_sum_kernel: the pooled power kernel with the cross-spectrum kernel's term between a row and
//                          the row before it -- X[t] conj(X[t - 1]) of one channel, the previous row of a chunk's first sample
//                          demodulated from the chunk's carry-in (sdft_hip_sdft_lag_sum_n)
//   sdft_forward_power_moments.hpp K1q forward_power_moments_kernel: the pooled power kernel with a second accumulator per bin -- the
//                          power and its square, each summed in registers over the windows of the grid and stored as a pair
//                          (sdft_hip_sdft_power_moments_n)
//   sdft_forward_covariance.hpp K1v forward_covariance_kernel: the cross-spectrum kernel with groups of channels in place of channels --
//                          all pairs of an array by register blocks of G x G pairs (sdft_hip_sdft_covariance_n)
//   sdft_forward_mix.hpp   K1m   forward_mix_kernel: forward_power_kernel's grid with the covariance kernel's groups of channels -- per-bin
//                          weighted sums of the windowed bins of the channels of a mix, for blocks of outputs (sdft_hip_sdft_mix_n)
//   sdft_forward_filterbank.hpp K1f forward_filterbank_kernel: the powers of a kept row go to a wave-private strip of LDS and the lanes
//                          form the weighted sums of the pieces of the plan's bands that lie in the tile; filterbank_rows_kernel adds
//                          the pieces of the bands a tile boundary cuts (sdft_hip_sdft_filterbank_n)
//   sdft_forward_band_peak.hpp K1b forward_band_peak_kernel: the filterbank kernel with numpy's argmax rule in the place of the sum --
//                          per piece the largest rounded product and its bin, as a pair; band_peak_rows_kernel joins the pieces of
//                          the bands a tile boundary cuts in ascending tile order by the same rule (sdft_hip_sdft_band_peak_n)
//   sdft_forward_hop.hpp   K1h   calls of one time chunk: forward_hop_kernel, forward_hop2_kernel (two waves per tile)
//   sdft_ops.hpp           spectral operations of the fused call, the synthesis term (sdft.h:641-651), user_rows_kernel
//   sdft_forward_rows.hpp  K1    forward_rows_kernel: one workgroup per (chunk, row), LDS edge exchange, lockstep row
//                          stores -- the dominant kernel; SYN != 0: fused synthesis on the windowed rows
//   sdft_fused.hpp         K3    fold_coeff_kernel, process_rows_kernel, process_hop2_kernel: analysis -> operation ->
//                          synthesis with window, operation and synthesis folded into one coefficient per bin
//   sdft_inverse.hpp       K2    inverse_exact_kernel (reference order, streaming), inverse_row_kernel (few rows),
//                          inverse_kernel (tree sum, with the rounding-interval proof of the reference's float), scale_rows_kernel
//
// Common decomposition: lanes <-> frequency bins (one complex bin per lane for 16-byte bins, two adjacent bins per lane
// for 8-byte bins, so a lane always stores 16 B), the sample loop is carried inside the kernel, the grid is
// bins x time chunks x channels.  The per-sample input difference is wave-uniform and arrives over the scalar unit
// (s_load through the constant address space); twiddles and state live in VGPRs for a whole chunk; window neighbours
// come from DPP whole-wave shifts (v_mov_b32_dpp wave_shr:1 / wave_shl:1).
//
// Arithmetic follows the reference's struct-complex formulas operation by operation and the translation units are
// compiled with -ffp-contract=off: given the same carry-in a wave reproduces the reference bit for bit (the FUSED
// instantiations of forward_rows_kernel and process_rows_kernel are the deliberate exceptions, used only where the
// carry-in already differs in summation order).
//
// This text is also compiled at run time, by hiprtc, for sdft_hip_process_n with sdft_hip_op_expr: build.py inlines the
// stage files into one string the library carries (the run-time compiler brings its own HIP declarations).

#pragma once

#include "sdft_base.hpp"
#include "sdft_carry_fast.hpp"
#include "sdft_carry_exact.hpp"
#include "sdft_forward.hpp"
#include "sdft_forward_every.hpp"
#include "sdft_forward_power.hpp"
#include "sdft_forward_power_sum.hpp"
#include "sdft_forward_power_peak.hpp"
#include "sdft_forward_power_smooth.hpp"
#include "sdft_forward_cross_sum.hpp"
#include "sdft_forward_cross_smooth.hpp"
#include "sdft_forward_smooth_peak.hpp"
#include "sdft_forward_lag_sum.hpp"
#include "sdft_forward_power_moments.hpp"
#include "sdft_forward_covariance.hpp"
#include "sdft_forward_mix.hpp"
#include "sdft_forward_filterbank.hpp"
#include "sdft_forward_band_peak.hpp"
#include "sdft_forward_hop.hpp"
#include "sdft_ops.hpp"
#include "sdft_forward_rows.hpp"
#include "sdft_fused.hpp"
#include "sdft_inverse.hpp"
