/*
 * host_smooth_peak.c -- a plain C host's noise-floor (or smoothed max-hold) tracker from a stream: the signal arrives in blocks
 * of `block` samples, each block is one sdft_hip_sdft_smooth_peak_n call on the windows of `every` samples; the smoothed power
 * travels from call to call in `state` together with sdft_hip_sdft_every_n's next first, and a call's head row completes the
 * last row of the call before it by the rule of sdft_hip.h.  Built by tests/test_gpu_smooth_peak.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_smooth_peak.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows, and the state behind the last of them, with the extreme over each window of the sequential
 * recursion over the oracle's powers of the whole signal.
 *
 * usage: host_smooth_peak <dftsize> <every> <block> <bin0> <nbins> <decay> <hold> <x.raw> <peaks.raw>
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
  if (argc < 10) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);
  const size_t block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]);
  const size_t nbins = (size_t)atol(argv[5]);
  const double decay = atof(argv[6]);
  const int hold = atoi(argv[7]);

  FILE* f = fopen(argv[8], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_smooth_peak_n(NULL, n, x, every, 0, bin0, nbins, decay, hold, NULL, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* windows of the whole signal (first = 0) */
  sdft_fd_t* peaks = (sdft_fd_t*)calloc((total + 1) * nbins, sizeof(sdft_fd_t));
  sdft_fd_t* part = (sdft_fd_t*)malloc((block / every + 2) * nbins * sizeof(sdft_fd_t));
  sdft_fd_t* state = (sdft_fd_t*)calloc(nbins, sizeof(sdft_fd_t));        /* the average starts from zero */

  /* every == 0, an empty band, a band past the last bin, a hold that is neither and a decay that never forgets are refused, and
     leave state alone */
  state[0] = (sdft_fd_t)7;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, 0, 0, bin0, nbins, decay, hold, state, part) != -1) return 6;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, every, 0, bin0, 0, decay, hold, state, part) != -1) return 6;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, every, 0, dftsize, 1, decay, hold, state, part) != -1) return 6;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, every, 0, bin0, nbins, decay, 2, state, part) != -1) return 6;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, every, 0, bin0, nbins, 1.0, hold, state, part) != -1) return 6;
  if (sdft_hip_sdft_smooth_peak_n(sdft, block, x, every, 0, bin0, nbins, -0.5, hold, state, part) != -1) return 6;
  if (state[0] != (sdft_fd_t)7) return 6;
  state[0] = (sdft_fd_t)0;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows of peaks begun so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const long rows = sdft_hip_sdft_smooth_peak_n(sdft, m, x + t, every, first, bin0, nbins, decay, hold, state, part);
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
  memcpy(peaks + total * nbins, state, nbins * sizeof(sdft_fd_t));       /* the state after the last sample, behind the rows */

  f = fopen(argv[9], "wb"); fwrite(peaks, sizeof(sdft_fd_t), (total + 1) * nbins, f); fclose(f);

  free(state); free(part); free(peaks); free(x);
  sdft_free(sdft);
  printf("C-HOST-SMOOTH-PEAK ok n=%zu rows=%zu calls=%zu hold=%d\n", n, total, calls, hold);
  return 0;
}
