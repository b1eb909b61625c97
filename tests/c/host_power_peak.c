/*
 * host_power_peak.c -- a plain C host's peak-hold (or minimum-hold) spectrogram from a stream: the signal arrives in blocks of
 * `block` samples, each block is one sdft_hip_sdft_power_peak_n call on the grid of `every` samples, and where a block boundary
 * cuts a window the next call's row 0 (its head) is combined into the previous call's last row by the call's own rule.  Built by
 * tests/test_gpu_power_peak.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_power_peak.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows with the extremes of the oracle's powers over the windows of the whole signal.
 *
 * usage: host_power_peak <dftsize> <every> <block> <bin0> <nbins> <hold> <x.raw> <peaks.raw>
 */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sdft/sdft.h>

/* the rule of sdft_hip.h: the extreme of the held value m and the term p; a NaN term stays */
static sdft_fd_t hold_rule(sdft_fd_t m, sdft_fd_t p, int hold)
{
  if (hold == sdft_hip_hold_min) return (p < m || p != p) ? p : m;
  return (p > m || p != p) ? p : m;
}

int main(int argc, char* argv[])
{
  if (argc < 9) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);
  const size_t block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]);
  const size_t nbins = (size_t)atol(argv[5]);
  const int hold = atoi(argv[6]);

  FILE* f = fopen(argv[7], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_power_peak_n(NULL, n, x, every, 0, bin0, nbins, hold, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* windows of the whole signal (first = 0) */
  sdft_fd_t* peaks = (sdft_fd_t*)calloc(total * nbins, sizeof(sdft_fd_t));
  sdft_fd_t* part = (sdft_fd_t*)malloc((block / every + 2) * nbins * sizeof(sdft_fd_t));

  /* every == 0, an empty band, a band past the last bin and a hold that is neither are refused */
  if (sdft_hip_sdft_power_peak_n(sdft, block, x, 0, 0, bin0, nbins, hold, part) != -1) return 6;
  if (sdft_hip_sdft_power_peak_n(sdft, block, x, every, 0, bin0, 0, hold, part) != -1) return 6;
  if (sdft_hip_sdft_power_peak_n(sdft, block, x, every, 0, dftsize, 1, hold, part) != -1) return 6;
  if (sdft_hip_sdft_power_peak_n(sdft, block, x, every, 0, bin0, nbins, 2, part) != -1) return 6;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows of peaks begun so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const long rows = sdft_hip_sdft_power_peak_n(sdft, m, x + t, every, first, bin0, nbins, hold, part);
    if (rows <= 0 || sdft_hip_last_error()) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
    size_t r = 0;
    if (first > 0)                                           /* row 0 is the head: it completes the last row begun */
    {
      if (done == 0) return 8;
      for (size_t k = 0; k < nbins; ++k) peaks[(done - 1) * nbins + k] = hold_rule(peaks[(done - 1) * nbins + k], part[k], hold);
      r = 1;
    }
    if (done + ((size_t)rows - r) > total) return 9;
    memcpy(peaks + done * nbins, part + r * nbins, ((size_t)rows - r) * nbins * sizeof(sdft_fd_t));
    done += (size_t)rows - r;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) { fprintf(stderr, "%zu rows of %zu\n", done, total); return 10; }

  f = fopen(argv[8], "wb"); fwrite(peaks, sizeof(sdft_fd_t), total * nbins, f); fclose(f);

  free(part); free(peaks); free(x);
  sdft_free(sdft);
  printf("C-HOST-POWER-PEAK ok n=%zu rows=%zu calls=%zu hold=%d\n", n, total, calls, hold);
  return 0;
}
