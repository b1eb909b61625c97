/*
 * host_covariance.c -- a plain C host's spatial covariance of a batched plan: channels x n samples, the array {2, 0, 1} installed
 * with sdft_hip_set_array, one sdft_hip_sdft_covariance_n call on the grid of `every` samples.  Built by
 * tests/test_gpu_covariance.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_covariance.c -lsdft_hip -lamdhip64 -lm
 * It prints an FNV-1a digest of the upper triangle's bytes, which the test compares with the digest of the Python call's result,
 * and the trace of the mirrored matrix of one bin against the sum of its diagonal elements.
 *
 * usage: host_covariance <dftsize> <channels> <every> <first> <bin0> <nbins> <x.raw>
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
  if (sdft_hip_sdft_covariance_n(NULL, n, x, every, first, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  if (sdft_hip_set_array(NULL, 0, NULL) != -1 || sdft_hip_array_channels(NULL) != 0) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_hip_alloc_batch(dftsize, sdft_window_hann, 1, channels);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t rows = (first > 0 ? 1 : 0) + (first < n ? (n - first + every - 1) / every : 0);
  const size_t nch = 3, T = nch * (nch + 1) / 2;
  const size_t chan[3] = {2, 0, 1};
  sdft_fdx_t* cov = (sdft_fdx_t*)calloc(T * rows * nbins, sizeof(sdft_fdx_t));

  /* no array yet; a channel the plan does not have, a repeated one, too many: refused, and the list stays as it was */
  if (sdft_hip_sdft_covariance_n(sdft, n, x, every, first, bin0, nbins, cov) != -1) return 6;
  const size_t far[2] = {0, channels}, twice[2] = {1, 1};
  if (sdft_hip_set_array(sdft, 2, far) != -1 || sdft_hip_set_array(sdft, 2, twice) != -1 || sdft_hip_set_array(sdft, channels + 1, NULL) != -1) return 6;
  if (sdft_hip_array_channels(sdft) != 0) return 6;
  sdft_hip_clear_error();
  if (sdft_hip_set_array(sdft, channels, NULL) != 0 || sdft_hip_array_channels(sdft) != channels) return 6;       /* NULL: 0 ... channels - 1 */
  if (sdft_hip_set_array(sdft, nch, chan) != 0 || sdft_hip_array_channels(sdft) != nch) { fprintf(stderr, "set_array: %s\n", sdft_hip_last_error()); return 6; }
  if (sdft_hip_set_array(sdft, 2, twice) != -1 || sdft_hip_array_channels(sdft) != nch) return 6;
  if (sdft_hip_sdft_covariance_n(sdft, n, x, 0, first, bin0, nbins, cov) != -1) return 6;
  sdft_hip_clear_error();

  const long got = sdft_hip_sdft_covariance_n(sdft, n, x, every, first, bin0, nbins, cov);
  if (got != (long)rows || sdft_hip_last_error()) { fprintf(stderr, "rows %ld of %zu: %s\n", got, rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }

  uint64_t h = 1469598103934665603ull;
  const unsigned char* bytes = (const unsigned char*)cov;
  for (size_t i = 0; i < T * rows * nbins * sizeof(sdft_fdx_t); ++i) { h ^= bytes[i]; h *= 1099511628211ull; }

  /* the matrix of the last row's first bin, mirrored: element (i, j), i <= j, is at i nch - i (i - 1) / 2 + (j - i) */
  const sdft_fd_t* s = (const sdft_fd_t*)cov;
  const size_t at = (rows - 1) * nbins;
  double trace = 0, imag_diag = 0, offdiag = 0;
  for (size_t i = 0; i < nch; ++i)
    for (size_t j = i; j < nch; ++j)
    {
      const size_t p = i * nch - i * (i - 1) / 2 + (j - i);
      const double re = s[2 * (p * rows * nbins + at)], im = s[2 * (p * rows * nbins + at) + 1];
      if (i == j) { trace += re; imag_diag += im < 0 ? -im : im; }
      else offdiag += re * re + im * im;
    }

  free(cov); free(x);
  sdft_free(sdft);
  printf("C-HOST-COVARIANCE ok n=%zu rows=%zu digest=%016llx trace=%.6e imagdiag=%.1e offdiag=%.6e\n", n, rows, (unsigned long long)h, trace, imag_diag, offdiag);
  return 0;
}
