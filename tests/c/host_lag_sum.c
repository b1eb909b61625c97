/*
 * host_lag_sum.c -- a plain C host's frequency tracker from a stream: the signal arrives in blocks of `block` samples, each block
 * is one sdft_hip_sdft_lag_sum_n call on the grid of `every` samples, and where a block boundary cuts a window the next call's
 * row 0 (its head) is added to the previous call's last row.  The row before a block's first sample is the plan's own state, so the
 * host keeps nothing between the calls but `first`.  Built by tests/test_gpu_lag_sum.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_lag_sum.c -lsdft_hip -lamdhip64 -lm
 * The test passes the sums it expects (the Python call in the same blocks) and the program compares them itself, bit for bit.
 *
 * usage: host_lag_sum <dftsize> <every> <block> <bin0> <nbins> <x.raw> <want.raw> <sums.raw>
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

  FILE* f = fopen(argv[6], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_lag_sum_n(NULL, n, x, every, 0, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* windows of the whole signal (first = 0) */
  const size_t row = 2 * nbins;                             /* numbers of a row: (re, im) per bin */
  sdft_fd_t* sums = (sdft_fd_t*)calloc(total * row, sizeof(sdft_fd_t));
  sdft_fd_t* part = (sdft_fd_t*)malloc((block / every + 2) * row * sizeof(sdft_fd_t));
  sdft_fd_t* want = (sdft_fd_t*)malloc(total * row * sizeof(sdft_fd_t));
  f = fopen(argv[7], "rb");
  if (!f || fread(want, sizeof(sdft_fd_t), total * row, f) != total * row) return 3;
  fclose(f);

  /* every == 0, an empty band, a band past the last bin and NULL sums are refused */
  if (sdft_hip_sdft_lag_sum_n(sdft, block, x, 0, 0, bin0, nbins, (sdft_fdx_t*)part) != -1) return 6;
  if (sdft_hip_sdft_lag_sum_n(sdft, block, x, every, 0, bin0, 0, (sdft_fdx_t*)part) != -1) return 6;
  if (sdft_hip_sdft_lag_sum_n(sdft, block, x, every, 0, dftsize, 1, (sdft_fdx_t*)part) != -1) return 6;
  if (sdft_hip_sdft_lag_sum_n(sdft, block, x, every, 0, bin0, nbins, NULL) != -1) return 6;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows of sums begun so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const long rows = sdft_hip_sdft_lag_sum_n(sdft, m, x + t, every, first, bin0, nbins, (sdft_fdx_t*)part);
    if (rows <= 0 || sdft_hip_last_error()) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
    size_t r = 0;
    if (first > 0)                                           /* row 0 is the head: it completes the last row begun */
    {
      if (done == 0) return 8;
      for (size_t k = 0; k < row; ++k) sums[(done - 1) * row + k] += part[k];
      r = 1;
    }
    if (done + ((size_t)rows - r) > total) return 9;
    memcpy(sums + done * row, part + r * row, ((size_t)rows - r) * row * sizeof(sdft_fd_t));
    done += (size_t)rows - r;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) { fprintf(stderr, "%zu rows of %zu\n", done, total); return 10; }

  f = fopen(argv[8], "wb"); fwrite(sums, sizeof(sdft_fd_t), total * row, f); fclose(f);
  size_t differ = 0;
  for (size_t i = 0; i < total * row; ++i) differ += memcmp(sums + i, want + i, sizeof(sdft_fd_t)) != 0;
  if (differ) { fprintf(stderr, "%zu of %zu numbers differ from the expected sums\n", differ, total * row); return 11; }

  free(want); free(part); free(sums); free(x);
  sdft_free(sdft);
  printf("C-HOST-LAG-SUM ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
