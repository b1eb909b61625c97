/*
 * host_cross_smooth.c -- a plain C host's recursive cross-spectrum of a two-channel stream: the signal arrives in blocks of
 * `block` samples per channel, each block is one sdft_hip_sdft_cross_smooth_n call on the grid of `every` samples for the pairs
 * (0,1), (1,0) and (1,1), and the averages travel from call to call in `state` together with sdft_hip_sdft_every_n's next first.
 * Built by tests/test_gpu_cross_smooth.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_cross_smooth.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows, and the state behind the last of them, with the sequential recursion over the oracle's rows of
 * the whole signal.
 *
 * usage: host_cross_smooth <dftsize> <every> <block> <bin0> <nbins> <decay> <x.raw> <smooth.raw>
 *        x.raw: [2][n] samples; smooth.raw: [3][rows + 1][nbins] complex, the state of a pair behind its rows
 */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sdft/sdft.h>

#define CHANNELS 2
#define NPAIRS 3

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
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t) / CHANNELS;
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(CHANNELS * n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), CHANNELS * n, f) != CHANNELS * n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_cross_smooth_n(NULL, n, x, every, 0, bin0, nbins, decay, NULL, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_hip_alloc_batch(dftsize, sdft_window_hann, 1, CHANNELS);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* rows of the whole signal (first = 0) */
  const size_t most = block / every + 2;                    /* rows of one call, at most */
  sdft_fdx_t* smooth = (sdft_fdx_t*)calloc(NPAIRS * (total + 1) * nbins, sizeof(sdft_fdx_t));
  sdft_fdx_t* piece = (sdft_fdx_t*)calloc(NPAIRS * most * nbins, sizeof(sdft_fdx_t));
  sdft_fdx_t* state = (sdft_fdx_t*)calloc(NPAIRS * nbins, sizeof(sdft_fdx_t));      /* the averages start from zero */
  sdft_td_t* xb = (sdft_td_t*)malloc(CHANNELS * block * sizeof(sdft_td_t));
  sdft_fd_t* first_number = (sdft_fd_t*)state;

  /* no pairs installed: refused */
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, every, 0, bin0, nbins, decay, state, piece) != -1) return 6;
  const size_t pa[NPAIRS] = {0, 1, 1}, pb[NPAIRS] = {1, 0, 1};
  if (sdft_hip_set_pairs(sdft, NPAIRS, pa, pb) != 0 || sdft_hip_pairs(sdft) != NPAIRS) { fprintf(stderr, "set_pairs: %s\n", sdft_hip_last_error()); return 6; }
  /* every == 0, an empty band, a band past the last bin and a decay that never forgets are refused, and leave state alone */
  first_number[0] = (sdft_fd_t)7;
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, 0, 0, bin0, nbins, decay, state, piece) != -1) return 6;
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, every, 0, bin0, 0, decay, state, piece) != -1) return 6;
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, every, 0, dftsize, 1, decay, state, piece) != -1) return 6;
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, every, 0, bin0, nbins, 1.0, state, piece) != -1) return 6;
  if (sdft_hip_sdft_cross_smooth_n(sdft, block, x, every, 0, bin0, nbins, -0.5, state, piece) != -1) return 6;
  if (first_number[0] != (sdft_fd_t)7) return 6;
  first_number[0] = (sdft_fd_t)0;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows written so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    if (done + grid > total || grid > most) return 9;
    for (size_t c = 0; c < CHANNELS; ++c) memcpy(xb + c * m, x + c * n + t, m * sizeof(sdft_td_t));      /* [channels][m] */
    /* a block without a grid point keeps no row (smooth may be NULL then) and still advances state */
    const long rows = sdft_hip_sdft_cross_smooth_n(sdft, m, xb, every, first, bin0, nbins, decay, state, grid ? piece : NULL);
    if (rows != (long)grid || sdft_hip_last_error()) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
    for (size_t p = 0; p < NPAIRS; ++p)                      /* the call's [npairs][grid][nbins] into the stream's [npairs][total + 1][nbins] */
      memcpy(smooth + (p * (total + 1) + done) * nbins, piece + p * grid * nbins, grid * nbins * sizeof(sdft_fdx_t));
    done += grid;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) { fprintf(stderr, "%zu rows of %zu\n", done, total); return 10; }
  for (size_t p = 0; p < NPAIRS; ++p)                        /* the state after the last sample, behind each pair's rows */
    memcpy(smooth + (p * (total + 1) + total) * nbins, state + p * nbins, nbins * sizeof(sdft_fdx_t));

  f = fopen(argv[8], "wb"); fwrite(smooth, sizeof(sdft_fdx_t), NPAIRS * (total + 1) * nbins, f); fclose(f);

  free(xb); free(state); free(piece); free(smooth); free(x);
  sdft_free(sdft);
  printf("C-HOST-CROSS-SMOOTH ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
