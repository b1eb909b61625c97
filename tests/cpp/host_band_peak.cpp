// host_band_peak.cpp -- a C++ host's band-peak calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): set_filterbank and
// band_peak.  The host feeds the signal in calls of ragged lengths on the grid of `every` samples, each call's first the documented
// one, and writes the rows of (value, bin) pairs of a small filterbank of overlapping bands; the test compares them with
// SDFT.band_peak of the whole signal in one call.  The checks of the host's own:
//   dftsize one-bin bands of weight 1 give power()'s every == 1 rows bit for bit, with bin k (a call of one time chunk);
//   a whole-row band's pair is the largest of those powers and the lowest bin that holds it;
//   a call without a filterbank throws.
// Built and run by tests/test_gpu_band_peak.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp.
//
// usage: host_band_peak <dftsize> <every> <x.raw> <rows.raw>

#include <sdft/sdft.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#ifndef HOST_T
#define HOST_T float
#endif
#ifndef HOST_F
#define HOST_F double
#endif

using sdft::SDFT;

int main(int argc, char* argv[])
{
  if (argc < 5) return 2;
  const size_t dftsize = (size_t)atol(argv[1]);
  const size_t every = (size_t)atol(argv[2]);

  FILE* f = fopen(argv[3], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(HOST_T);
  fseek(f, 0, SEEK_SET);
  std::vector<HOST_T> x(n);
  if (fread(x.data(), sizeof(HOST_T), n, f) != n) return 3;
  fclose(f);

  SDFT<HOST_T, HOST_F> sdft(dftsize, sdft::Window::Hann, 1);
  const size_t m = sdft.size();
  if (m != dftsize || sdft.filterbank_bands() != 0) return 4;

  // no filterbank: the call says so
  bool thrown = false;
  std::vector<HOST_F> none(2);
  try { sdft.band_peak(1, x.data(), 1, 0, none.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_band_peak_n") != nullptr; }
  if (!thrown) return 5;

  // the powers of the first rows: a call of one time chunk
  const size_t head = n < 441 ? n : 441;
  std::vector<HOST_F> p(head * m);
  if (sdft.power(head, x.data(), 1, 0, 0, m, p.data()) != head) return 6;

  // one band per bin, weight 1: the powers bit for bit, bin k
  const std::vector<HOST_F> ones(m, (HOST_F)1);
  std::vector<size_t> bin0(m), nbins(m, 1);
  for (size_t k = 0; k < m; ++k) bin0[k] = k;
  sdft.set_filterbank(m, bin0.data(), nbins.data(), ones.data());
  if (sdft.filterbank_bands() != m) return 7;
  std::vector<HOST_F> each(head * m * 2);
  sdft.reset();
  if (sdft.band_peak(head, x.data(), 1, 0, each.data()) != head) return 8;
  for (size_t r = 0; r < head; ++r)
    for (size_t k = 0; k < m; ++k)
    {
      if (memcmp(&each[(r * m + k) * 2], &p[r * m + k], sizeof(HOST_F)) != 0) { fprintf(stderr, "row %zu bin %zu: value\n", r, k); return 9; }
      if (each[(r * m + k) * 2 + 1] != (HOST_F)k) { fprintf(stderr, "row %zu bin %zu: bin %g\n", r, k, (double)each[(r * m + k) * 2 + 1]); return 9; }
    }

  // one band over the whole row: the largest power and the lowest bin that holds it
  const size_t row_bin0 = 0, row_nbins = m;
  sdft.set_filterbank(1, &row_bin0, &row_nbins, ones.data());
  std::vector<HOST_F> whole(head * 2);
  sdft.reset();
  if (sdft.band_peak(head, x.data(), 1, 0, whole.data()) != head) return 10;
  for (size_t r = 0; r < head; ++r)
  {
    size_t at = 0;
    for (size_t k = 1; k < m; ++k) if (p[r * m + k] > p[r * m + at]) at = k;
    if (memcmp(&whole[r * 2], &p[r * m + at], sizeof(HOST_F)) != 0 || whole[r * 2 + 1] != (HOST_F)at)
    { fprintf(stderr, "row %zu: (%g, %g), expected (%g, %zu)\n", r, (double)whole[r * 2], (double)whole[r * 2 + 1], (double)p[r * m + at], at); return 11; }
  }

  // the stream: band b from bin b * dftsize / 32 on, dftsize / 8 + 7 b bins (cut at the last bin); weights are multiples of 1/16
  const size_t NBANDS = 24;
  std::vector<size_t> b0(NBANDS), nb(NBANDS);
  std::vector<HOST_F> w;
  for (size_t b = 0; b < NBANDS; ++b)
  {
    b0[b] = b * dftsize / 32;
    nb[b] = dftsize / 8 + 7 * b;
    if (nb[b] > dftsize - b0[b]) nb[b] = dftsize - b0[b];
    for (size_t k = 0; k < nb[b]; ++k) w.push_back((HOST_F)(1 + (b * 31 + k * 7) % 13) / 16 - (HOST_F)0.25);
  }
  sdft.set_filterbank(NBANDS, b0.data(), nb.data(), w.data());
  sdft.reset();
  const size_t total_rows = (n + every - 1) / every;         // rows of the whole signal (first = 0)
  std::vector<HOST_F> rows(total_rows * NBANDS * 2);
  static const size_t lengths[] = {1, 730, 99, 512, 1300, 2, 513};
  size_t done = 0, first = 0, calls = 0;                     // rows written so far; the next call's first
  for (size_t t = 0; t < n; ++calls)
  {
    size_t k = lengths[calls % (sizeof(lengths) / sizeof(lengths[0]))];
    if (k > n - t) k = n - t;
    const size_t expect = first < k ? (k - first - 1) / every + 1 : 0;
    if (done + expect > total_rows) return 12;
    if (sdft.band_peak(k, x.data() + t, every, first, expect ? rows.data() + done * NBANDS * 2 : nullptr) != expect) return 13;
    done += expect;
    first = expect ? first + expect * every - k : first - k; // the grid goes on where it left off
    t += k;
  }
  if (done != total_rows) return 14;

  f = fopen(argv[4], "wb");
  if (!f) return 3;
  fwrite(rows.data(), sizeof(HOST_F), rows.size(), f);
  fclose(f);
  printf("CPP-BAND-PEAK ok n=%zu m=%zu rows=%zu calls=%zu\n", n, m, total_rows, calls);
  return 0;
}
