/*
 * host_band_peak.c -- a plain C host's band peaks from a stream: it installs a small filterbank of overlapping bands, most of them
 * wider than a tile of the plan (so they are split), feeds the signal in calls of ragged lengths on the grid of `every` samples --
 * each call's first is the documented one: the grid goes on where the previous call left it -- and writes the rows of (value, bin)
 * pairs.
 * Built by tests/test_gpu_band_peak.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_band_peak.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows with SDFT.band_peak of the whole signal in one call (the same bands and weights).
 *
 * usage: host_band_peak <dftsize> <every> <x.raw> <rows.raw>
 */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sdft/sdft.h>

#define NBANDS 24

int main(int argc, char* argv[])
{
  if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);

  FILE* f = fopen(argv[3], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* band b: from bin b * dftsize / 32 on, dftsize / 8 + 7 b bins (cut at the last bin); weights are multiples of 1/16 */
  sdft_size_t bin0[NBANDS], nbins[NBANDS];
  size_t total = 0;
  for (size_t b = 0; b < NBANDS; ++b)
  {
    bin0[b] = b * dftsize / 32;
    nbins[b] = dftsize / 8 + 7 * b;
    if (nbins[b] > dftsize - bin0[b]) nbins[b] = dftsize - bin0[b];
    total += nbins[b];
  }
  sdft_fd_t* w = (sdft_fd_t*)malloc(total * sizeof(sdft_fd_t));
  for (size_t b = 0, at = 0; b < NBANDS; ++b)
    for (size_t k = 0; k < nbins[b]; ++k) w[at++] = (sdft_fd_t)(1 + (b * 31 + k * 7) % 13) / 16 - (sdft_fd_t)0.25;

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_band_peak_n(NULL, n, x, every, 0, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total_rows = (n + every - 1) / every;         /* rows of the whole signal (first = 0) */
  sdft_fd_t* rows = (sdft_fd_t*)calloc(total_rows * NBANDS * 2, sizeof(sdft_fd_t));

  /* no filterbank installed yet */
  if (sdft_hip_filterbank_bands(sdft) != 0) return 6;
  if (sdft_hip_sdft_band_peak_n(sdft, 100, x, every, 0, rows) != -1) return 6;
  if (!sdft_hip_last_error() || !strstr(sdft_hip_last_error(), "sdft_hip_sdft_band_peak_n") || !strstr(sdft_hip_last_error(), "filterbank")) return 6;
  sdft_hip_clear_error();

  if (sdft_hip_set_filterbank(sdft, NBANDS, bin0, nbins, w) != 0) { fprintf(stderr, "set_filterbank: %s\n", sdft_hip_last_error()); return 7; }
  if (sdft_hip_filterbank_bands(sdft) != NBANDS || sdft_hip_last_error()) return 7;

  /* every == 0 and NULL peaks with rows to write are refused */
  if (sdft_hip_sdft_band_peak_n(sdft, 100, x, 0, 0, rows) != -1) return 8;
  if (!sdft_hip_last_error() || !strstr(sdft_hip_last_error(), "every")) return 8;
  sdft_hip_clear_error();
  if (sdft_hip_sdft_band_peak_n(sdft, 100, x, every, 0, NULL) != -1) return 8;
  if (!sdft_hip_last_error() || !strstr(sdft_hip_last_error(), "NULL")) return 8;
  sdft_hip_clear_error();

  static const size_t lengths[] = {1, 730, 99, 512, 1300, 2, 513};
  size_t done = 0, first = 0, calls = 0;                     /* rows written so far; the next call's first */
  for (size_t t = 0; t < n; ++calls)
  {
    size_t m = lengths[calls % (sizeof(lengths) / sizeof(lengths[0]))];
    if (m > n - t) m = n - t;
    const size_t expect = first < m ? (m - first - 1) / every + 1 : 0;
    if (done + expect > total_rows) return 9;
    const long got = sdft_hip_sdft_band_peak_n(sdft, m, x + t, every, first, expect ? rows + done * NBANDS * 2 : NULL);
    if (got != (long)expect || sdft_hip_last_error()) { fprintf(stderr, "rows %ld of %zu: %s\n", got, expect, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 10; }
    done += expect;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    first = expect ? first + expect * every - m : first - m;
    t += m;
  }
  if (done != total_rows) { fprintf(stderr, "%zu rows of %zu\n", done, total_rows); return 11; }

  /* every bin is an integer inside its band */
  for (size_t r = 0; r < total_rows; ++r)
    for (size_t b = 0; b < NBANDS; ++b)
    {
      const sdft_fd_t bin = rows[(r * NBANDS + b) * 2 + 1];
      if (bin != (sdft_fd_t)(size_t)bin || (size_t)bin < bin0[b] || (size_t)bin >= bin0[b] + nbins[b]) { fprintf(stderr, "row %zu band %zu: bin %g\n", r, b, (double)bin); return 12; }
    }

  f = fopen(argv[4], "wb"); fwrite(rows, sizeof(sdft_fd_t), total_rows * NBANDS * 2, f); fclose(f);

  free(rows); free(w); free(x);
  sdft_free(sdft);
  printf("C-HOST-BAND-PEAK ok n=%zu rows=%zu calls=%zu\n", n, total_rows, calls);
  return 0;
}
