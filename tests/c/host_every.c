/*
 * host_every.c -- a plain C host that keeps what the reference's test driver keeps (test/test.c: sdft_sdft_n on hops of
 * `hop` samples, row 0 of each hop copied out) with ONE sdft_hip_sdft_every_n call over the whole signal.  Built by
 * tests/test_gpu_every.py with
 *   gcc -std=c99 -Iinclude [-DSDFT_FD_FLOAT] host_every.c -lsdft_hip -lamdhip64 -lm
 * The test compares the rows with the oracle.
 *
 * usage: host_every <dftsize> <hop> <x.raw> <dft.raw>
 */

#include <stdio.h>
#include <stdlib.h>

#include <sdft/sdft.h>

int main(int argc, char* argv[])
{
  if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t hop = (size_t)atol(argv[2]);

  FILE* f = fopen(argv[3], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  size_t n = (size_t)ftell(f) / sizeof(sdft_td_t);
  fseek(f, 0, SEEK_SET);
  sdft_td_t* x = (sdft_td_t*)malloc(n * sizeof(sdft_td_t));
  if (fread(x, sizeof(sdft_td_t), n, f) != n) return 3;
  fclose(f);
  n = (n / hop) * hop;

  /* a NULL plan is refused with an error text */
  if (sdft_hip_sdft_every_n(NULL, n, x, hop, 0, NULL) != -1 || !sdft_hip_last_error()) return 4;
  sdft_hip_clear_error();

  sdft_t* sdft = sdft_alloc_custom(dftsize, sdft_window_hann, 1);
  if (!sdft) { fprintf(stderr, "alloc failed: %s\n", sdft_hip_last_error()); return 5; }

  /* every == 0 is refused */
  sdft_fdx_t* dfts = (sdft_fdx_t*)malloc((n / hop) * dftsize * sizeof(sdft_fdx_t));
  if (sdft_hip_sdft_every_n(sdft, n, x, 0, 0, dfts) != -1) return 6;
  sdft_hip_clear_error();

  const long rows = sdft_hip_sdft_every_n(sdft, n, x, hop, 0, dfts);
  if (rows != (long)(n / hop)) { fprintf(stderr, "rows %ld: %s\n", rows, sdft_hip_last_error() ? sdft_hip_last_error() : ""); return 7; }
  if (sdft_hip_last_error()) { fprintf(stderr, "error: %s\n", sdft_hip_last_error()); return 8; }

  f = fopen(argv[4], "wb"); fwrite(dfts, sizeof(sdft_fdx_t), (size_t)rows * dftsize, f); fclose(f);

  free(dfts); free(x);
  sdft_free(sdft);
  printf("C-HOST-EVERY ok n=%zu rows=%ld\n", n, rows);
  return 0;
}
