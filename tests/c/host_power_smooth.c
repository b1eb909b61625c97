/*
 * host_power_smooth.c -- a plain C host's exponentially averaged spectrogram from a stream: the signal arrives in blocks of
 * `block` samples, each block is one sdft_hip_sdft_power_smooth_n call on the grid of `every` samples, and the average travels
 * from call to call in `state` together with sdft_hip_sdft_every_n's next first.  Built by tests/test_gpu_power_smooth.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_power_smooth.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows, and the state behind the last of them, with the sequential recursion over the oracle's powers of
 * the whole signal.
 *
 * usage: host_power_smooth <dftsize> <every> <block> <bin0> <nbins> <decay> <x.raw> <smooth.raw>
 */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 9) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);
  const size_t block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]);
  const size_t nbins = (size_t)atol(argv[5]);
  const double decay = atof(argv[6]);

  FILE* f = fopen(argv[7], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_power_smooth_n(NULL, n, x, every, 0, bin0, nbins, decay, NULL, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* rows of the whole signal (first = 0) */
  sdft_fd_t* smooth = (sdft_fd_t*)calloc((total + 1) * nbins, sizeof(sdft_fd_t));
  sdft_fd_t* state = (sdft_fd_t*)calloc(nbins, sizeof(sdft_fd_t));        /* the average starts from zero */

  /* every == 0, an empty band, a band past the last bin and a decay that never forgets are refused, and leave state alone */
  state[0] = (sdft_fd_t)7;
  if (sdft_hip_sdft_power_smooth_n(sdft, block, x, 0, 0, bin0, nbins, decay, state, smooth) != -1) return 6;
  if (sdft_hip_sdft_power_smooth_n(sdft, block, x, every, 0, bin0, 0, decay, state, smooth) != -1) return 6;
  if (sdft_hip_sdft_power_smooth_n(sdft, block, x, every, 0, dftsize, 1, decay, state, smooth) != -1) return 6;
  if (sdft_hip_sdft_power_smooth_n(sdft, block, x, every, 0, bin0, nbins, 1.0, state, smooth) != -1) return 6;
  if (sdft_hip_sdft_power_smooth_n(sdft, block, x, every, 0, bin0, nbins, -0.5, state, smooth) != -1) return 6;
  if (state[0] != (sdft_fd_t)7) return 6;
  state[0] = (sdft_fd_t)0;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows written so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    if (done + grid > total) return 9;
    /* a block without a grid point keeps no row (smooth may be NULL then) and still advances state */
    const long rows = sdft_hip_sdft_power_smooth_n(sdft, m, x + t, every, first, bin0, nbins, decay, state, grid ? smooth + done * nbins : NULL);
    if (rows != (long)grid || sdft_hip_last_error()) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
    done += grid;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) { fprintf(stderr, "%zu rows of %zu\n", done, total); return 10; }
  memcpy(smooth + total * nbins, state, nbins * sizeof(sdft_fd_t));      /* the state after the last sample, behind the rows */

  f = fopen(argv[8], "wb"); fwrite(smooth, sizeof(sdft_fd_t), (total + 1) * nbins, f); fclose(f);

  free(state); free(smooth); free(x);
  sdft_free(sdft);
  printf("C-HOST-POWER-SMOOTH ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
