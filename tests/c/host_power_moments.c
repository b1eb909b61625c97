/*
 * host_power_moments.c -- a plain C host's power moments from a stream: the signal arrives in blocks of `block` samples, each
 * block is one sdft_hip_sdft_power_moments_n call on the grid of `every` samples, and where a block boundary cuts a window the next
 * call's row 0 (its head) is added, both components, to the previous call's last row.  Built by tests/test_gpu_power_moments.py
 * with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_power_moments.c -lsdft_hip -lamdhip64 -lm
 * The test compares the pairs with the sums of the oracle's powers and of their squares over the windows of the whole signal, and
 * with the Python call's bits.
 *
 * usage: host_power_moments <dftsize> <every> <block> <bin0> <nbins> <x.raw> <moments.raw>
 */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 8) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);
  const size_t block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]);
  const size_t nbins = (size_t)atol(argv[5]);
  const size_t pair = 2 * nbins;                             /* numbers per row: (s1, s2) per bin */

  FILE* f = fopen(argv[6], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_power_moments_n(NULL, n, x, every, 0, bin0, nbins, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  const size_t total = (n + every - 1) / every;             /* windows of the whole signal (first = 0) */
  sdft_fd_t* moments = (sdft_fd_t*)calloc(total * pair, sizeof(sdft_fd_t));
  sdft_fd_t* part = (sdft_fd_t*)malloc((block / every + 2) * pair * sizeof(sdft_fd_t));

  /* every == 0, an empty band, a band past the last bin and a NULL output are refused */
  if (sdft_hip_sdft_power_moments_n(sdft, block, x, 0, 0, bin0, nbins, part) != -1) return 6;
  if (sdft_hip_sdft_power_moments_n(sdft, block, x, every, 0, bin0, 0, part) != -1) return 6;
  if (sdft_hip_sdft_power_moments_n(sdft, block, x, every, 0, dftsize, 1, part) != -1) return 6;
  if (sdft_hip_sdft_power_moments_n(sdft, block, x, every, 0, bin0, nbins, NULL) != -1) return 6;
  sdft_hip_clear_error();

  size_t done = 0, first = 0, calls = 0;                    /* rows of moments begun so far; the next call's first */
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const long rows = sdft_hip_sdft_power_moments_n(sdft, m, x + t, every, first, bin0, nbins, part);
    if (rows <= 0 || sdft_hip_last_error()) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
    size_t r = 0;
    if (first > 0)                                           /* row 0 is the head: it completes the last row begun */
    {
      if (done == 0) return 8;
      for (size_t k = 0; k < pair; ++k) moments[(done - 1) * pair + k] = moments[(done - 1) * pair + k] + part[k];
      r = 1;
    }
    if (done + ((size_t)rows - r) > total) return 9;
    memcpy(moments + done * pair, part + r * pair, ((size_t)rows - r) * pair * sizeof(sdft_fd_t));
    done += (size_t)rows - r;
    /* the next call's first, as for sdft_hip_sdft_every_n: the grid goes on where it left off */
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) { fprintf(stderr, "%zu rows of %zu\n", done, total); return 10; }

  /* the variance of the power of the first window's first bin: s2 / L - (s1 / L)^2, never negative beyond rounding */
  const double L = (double)(n < every ? n : every);
  const double mean = (double)moments[0] / L, var = (double)moments[1] / L - mean * mean;
  if (!(var >= -1e-6 * mean * mean)) { fprintf(stderr, "variance %g of mean %g\n", var, mean); return 11; }

  f = fopen(argv[7], "wb"); fwrite(moments, sizeof(sdft_fd_t), total * pair, f); fclose(f);

  free(part); free(moments); free(x);
  sdft_free(sdft);
  printf("C-HOST-POWER-MOMENTS ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
