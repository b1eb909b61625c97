/*
 * host_cross_sum.c -- a plain C host's cross-spectra of a batched plan: channels x n samples, the pairs (0,0), (1,1), (0,1) and
 * (2,0) installed with sdft_hip_set_pairs, one sdft_hip_sdft_cross_sum_n call on the grid of `every` samples.  Built by
 * tests/test_gpu_cross_sum.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_cross_sum.c -lsdft_hip -lamdhip64 -lm
 * It prints an FNV-1a digest of the sums' bytes, which the test compares with the digest of the Python call's result, and the
 * magnitude-squared coherence of the channels 0 and 1 in one bin.
 *
 * usage: host_cross_sum <dftsize> <channels> <every> <first> <bin0> <nbins> <x.raw>
 */

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 8) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t channels = (size_t)atol(argv[2]);
  const size_t every = (size_t)atol(argv[3]);
  const size_t first = (size_t)atol(argv[4]);
  const size_t bin0 = (size_t)atol(argv[5]);
  const size_t nbins = (size_t)atol(argv[6]);

  FILE* f = fopen(argv[7], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t) / channels;
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(channels * n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), channels * n, f) != channels * n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_cross_sum_n(NULL, n, x, every, first, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  if (sdft_hip_set_pairs(NULL, 0, NULL, NULL) != -1 || sdft_hip_pairs(NULL) != 0) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_hip_alloc_batch(dftsize, sdft_window_hann, 1, channels);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t rows = (first > 0 ? 1 : 0) + (first < n ? (n - first + every - 1) / every : 0);
  const size_t pa[4] = {0, 1, 0, 2}, pb[4] = {0, 1, 1, 0};
  sdft_fdx_t* sums = (sdft_fdx_t*)calloc(4 * rows * nbins, sizeof(sdft_fdx_t));

  /* no pairs yet, a channel the plan does not have: refused, and the list stays as it was */
  if (sdft_hip_sdft_cross_sum_n(sdft, n, x, every, first, bin0, nbins, sums) != -1) return 6;
  const size_t bad[1] = {channels};
  if (sdft_hip_set_pairs(sdft, 1, pa, bad) != -1 || sdft_hip_pairs(sdft) != 0) return 6;
  sdft_hip_clear_error();
  if (sdft_hip_set_pairs(sdft, 4, pa, pb) != 0 || sdft_hip_pairs(sdft) != 4) { fprintf(stderr, "set_pairs: %s\n", sdft_hip_last_error()); return 6; }
  if (sdft_hip_set_pairs(sdft, 1, pa, bad) != -1 || sdft_hip_pairs(sdft) != 4) return 6;
  if (sdft_hip_sdft_cross_sum_n(sdft, n, x, 0, first, bin0, nbins, sums) != -1) return 6;
  sdft_hip_clear_error();

  const long got = sdft_hip_sdft_cross_sum_n(sdft, n, x, every, first, bin0, nbins, sums);
  if (got != (long)rows || sdft_hip_last_error()) { fprintf(stderr, "rows %ld of %zu: %s\n", got, rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }

  uint64_t h = 1469598103934665603ull;
  const unsigned char* bytes = (const unsigned char*)sums;
  for (size_t i = 0; i < 4 * rows * nbins * sizeof(sdft_fdx_t); ++i) { h ^= bytes[i]; h *= 1099511628211ull; }

  /* coherence |S_01|^2 / (S_00 S_11) of the last row's first bin */
  const sdft_fd_t* s = (const sdft_fd_t*)sums;
  const size_t at = (rows - 1) * nbins;
  const double s00 = s[2 * (0 * rows * nbins + at)], s11 = s[2 * (1 * rows * nbins + at)];
  const double re = s[2 * (2 * rows * nbins + at)], im = s[2 * (2 * rows * nbins + at) + 1];
  const double coherence = s00 > 0 && s11 > 0 ? (re * re + im * im) / (s00 * s11) : 0.0;

  free(sums); free(x);
  sdft_free(sdft);
  printf("C-HOST-CROSS-SUM ok n=%zu rows=%zu digest=%016llx coherence=%.6f\n", n, rows, (unsigned long long)h, coherence);
  return 0;
}
