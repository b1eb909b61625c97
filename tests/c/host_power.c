/*
 * host_power.c -- a plain C host's spectrogram: the power of the bins [bin0, bin0 + nbins) every `hop` samples, from ONE
 * sdft_hip_sdft_power_n call over the whole signal into host memory.  Built by tests/test_gpu_power.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_power.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows with re*re + im*im of the oracle's rows.
 *
 * usage: host_power <dftsize> <hop> <bin0> <nbins> <x.raw> <power.raw>
 */

#include <stdio.h>
#include <stdlib.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 7) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t hop = (size_t)atol(argv[2]);
  const size_t bin0 = (size_t)atol(argv[3]);
  const size_t nbins = (size_t)atol(argv[4]);

  FILE* f = fopen(argv[5], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);
  n = (n / hop) * hop;

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_power_n(NULL, n, x, hop, 0, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  /* every == 0, an empty band and a band past the last bin are refused */
  sdft_fd_t* power = (sdft_fd_t*)malloc((n / hop) * nbins * sizeof(sdft_fd_t));
  if (sdft_hip_sdft_power_n(sdft, n, x, 0, 0, bin0, nbins, power) != -1) return 6;
  if (sdft_hip_sdft_power_n(sdft, n, x, hop, 0, bin0, 0, power) != -1) return 6;
  if (sdft_hip_sdft_power_n(sdft, n, x, hop, 0, dftsize, 1, power) != -1) return 6;
  if (sdft_hip_sdft_power_n(sdft, n, x, hop, 0, 1, (size_t)-1, power) != -1) return 6;
  sdft_hip_clear_error();

  const long rows = sdft_hip_sdft_power_n(sdft, n, x, hop, 0, bin0, nbins, power);
  if (rows != (long)(n / hop)) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
  if (sdft_hip_last_error()) { fprintf(stderr, "error: %s\n", sdft_hip_last_error()); return 8; }

  f = fopen(argv[6], "wb"); fwrite(power, sizeof(sdft_fd_t), (size_t)rows * nbins, f); fclose(f);

  free(power); free(x);
  sdft_free(sdft);
  printf("C-HOST-POWER ok n=%zu rows=%ld\n", n, rows);
  return 0;
}
