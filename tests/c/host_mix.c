/*
 * host_mix.c -- a plain C host's channel mix of a batched plan: channels x n samples, the mix {2, 0, 1} with two outputs installed
 * with sdft_hip_set_mix from a file of weights [2][3][dftsize], one sdft_hip_sdft_mix_n call on the grid of `every` samples.  Built
 * by tests/test_gpu_mix.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_mix.c -lsdft_hip -lamdhip64 -lm
 * It writes the rows [2][rows][nbins] to a file, which the test compares with the Python call's result bit for bit.
 *
 * usage: host_mix <dftsize> <channels> <every> <first> <bin0> <nbins> <x.raw> <w.raw> <y.raw>
 */

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 10) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t channels = (size_t)atol(argv[2]);
  const size_t every = (size_t)atol(argv[3]);
  const size_t first = (size_t)atol(argv[4]);
  const size_t bin0 = (size_t)atol(argv[5]);
  const size_t nbins = (size_t)atol(argv[6]);
  const size_t nout = 2, nch = 3;
  const size_t chan[3] = {2, 0, 1};

  FILE* f = fopen(argv[7], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t) / channels;
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(channels * n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), channels * n, f) != channels * n) return 3;
  fclose(f);
  sdft_fdx_t* w = (sdft_fdx_t*)malloc(nout * nch * dftsize * sizeof(sdft_fdx_t));
  f = fopen(argv[8], "rb");
  if (!f || fread(w, sizeof(sdft_fdx_t), nout * nch * dftsize, f) != nout * nch * dftsize) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_mix_n(NULL, n, x, every, first, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  if (sdft_hip_set_mix(NULL, 0, 0, NULL, NULL) != -1 || sdft_hip_mix_outputs(NULL) != 0) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_hip_alloc_batch(dftsize, sdft_window_hann, 1, channels);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t rows = first < n ? (n - first + every - 1) / every : 0;
  sdft_fdx_t* y = (sdft_fdx_t*)calloc(nout * rows * nbins, sizeof(sdft_fdx_t));

  /* no mix yet; a channel the plan does not have, a repeated one, too many, no weights, no channels: refused, nothing installed */
  if (sdft_hip_sdft_mix_n(sdft, n, x, every, first, bin0, nbins, y) != -1) return 6;
  const size_t far[2] = {0, channels}, twice[2] = {1, 1};
  if (sdft_hip_set_mix(sdft, 1, 2, far, w) != -1 || sdft_hip_set_mix(sdft, 1, 2, twice, w) != -1 || sdft_hip_set_mix(sdft, 1, channels + 1, NULL, w) != -1) return 6;
  if (sdft_hip_set_mix(sdft, 1, 2, NULL, NULL) != -1 || sdft_hip_set_mix(sdft, 1, 0, NULL, w) != -1) return 6;
  if (sdft_hip_mix_outputs(sdft) != 0) return 6;
  sdft_hip_clear_error();
  if (sdft_hip_set_mix(sdft, 1, nch, NULL, w) != 0 || sdft_hip_mix_outputs(sdft) != 1) return 6;       /* NULL: 0 ... nch - 1 */
  if (sdft_hip_set_mix(sdft, nout, nch, chan, w) != 0 || sdft_hip_mix_outputs(sdft) != nout) { fprintf(stderr, "set_mix: %s\n", sdft_hip_last_error()); return 6; }
  if (sdft_hip_set_mix(sdft, 1, 2, twice, w) != -1 || sdft_hip_mix_outputs(sdft) != nout) return 6;
  if (sdft_hip_sdft_mix_n(sdft, n, x, 0, first, bin0, nbins, y) != -1) return 6;
  sdft_hip_clear_error();

  const long got = sdft_hip_sdft_mix_n(sdft, n, x, every, first, bin0, nbins, y);
  if (got != (long)rows || sdft_hip_last_error()) { fprintf(stderr, "rows %ld of %zu: %s\n", got, rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }

  f = fopen(argv[9], "wb");
  if (!f || fwrite(y, sizeof(sdft_fdx_t), nout * rows * nbins, f) != nout * rows * nbins) return 8;
  fclose(f);

  if (sdft_hip_set_mix(sdft, 0, 0, NULL, NULL) != 0 || sdft_hip_mix_outputs(sdft) != 0) return 9;

  free(y); free(w); free(x);
  sdft_free(sdft);
  printf("C-HOST-MIX ok n=%zu rows=%zu\n", n, rows);
  return 0;
}
