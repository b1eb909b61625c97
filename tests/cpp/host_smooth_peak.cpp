// host_smooth_peak.cpp -- a C++ host's smoothed peak-hold calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): a stream in blocks
// of `block` samples on the windows of `every` samples, the smoothed power passed from call to call in `state`, head rows joined
// by the rule.  The host's own checks:
//   decay 0 on a twin plan is power_peak()'s rows bit for bit;
//   a decay of 1 throws, with the call's name in the text, and leaves state alone.
// Built and run by tests/test_gpu_smooth_peak.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp; the test compares
// the file -- the rows, then the state after the last sample -- with the extreme over each window of the sequential recursion
// over the oracle's powers.
//
// usage: host_smooth_peak <dftsize> <every> <block> <bin0> <nbins> <decay> <hold> <x.raw> <peaks.raw>

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

static HOST_F hold_rule(HOST_F m, HOST_F p, sdft::Hold hold)
{
  if (hold == sdft::Hold::Min) return (p < m || p != p) ? p : m;
  return (p > m || p != p) ? p : m;
}

int main(int argc, char* argv[])
{
  if (argc < 10) return 2;
  const size_t dftsize = (size_t)atol(argv[1]), every = (size_t)atol(argv[2]), block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]), nbins = (size_t)atol(argv[5]);
  const double decay = atof(argv[6]);
  const sdft::Hold hold = atoi(argv[7]) ? sdft::Hold::Min : sdft::Hold::Max;

  FILE* f = fopen(argv[8], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(HOST_T);
  fseek(f, 0, SEEK_SET);
  std::vector<HOST_T> x(n);
  if (fread(x.data(), sizeof(HOST_T), n, f) != n) return 3;
  fclose(f);

  SDFT<HOST_T, HOST_F> sdft(dftsize, sdft::Window::Hann, 1), zero(dftsize, sdft::Window::Hann, 1), twin(dftsize, sdft::Window::Hann, 1);
  if (sdft.size() != dftsize) return 4;

  const size_t total = (n + every - 1) / every;
  const size_t most = (block / every + 2) * nbins;
  std::vector<HOST_F> peaks((total + 1) * nbins), state(nbins, (HOST_F)0), part(most), a(most), b(most);

  bool thrown = false;
  state[0] = (HOST_F)7;
  try { sdft.smooth_peak(block, x.data(), every, 0, bin0, nbins, 1.0, hold, state.data(), part.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_smooth_peak_n") != nullptr; }
  if (!thrown || state[0] != (HOST_F)7) return 5;
  state[0] = (HOST_F)0;

  size_t done = 0, first = 0, calls = 0;
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t rows = sdft.smooth_peak(m, x.data() + t, every, first, bin0, nbins, decay, hold, state.data(), part.data());
    if (rows == 0) return 6;
    // decay 0 forgets at once: power_peak()'s rows, bit for bit, with or without a state
    if (zero.smooth_peak(m, x.data() + t, every, first, bin0, nbins, 0.0, hold, nullptr, a.data()) != rows ||
        twin.power_peak(m, x.data() + t, every, first, bin0, nbins, hold, b.data()) != rows) return 7;
    if (memcmp(a.data(), b.data(), rows * nbins * sizeof(HOST_F)) != 0) { fprintf(stderr, "call %zu: decay 0 is not power_peak()\n", calls); return 8; }
    size_t r = 0;
    if (first > 0)
    {
      if (done == 0) return 8;
      for (size_t k = 0; k < nbins; ++k) peaks[(done - 1) * nbins + k] = hold_rule(peaks[(done - 1) * nbins + k], part[k], hold);
      r = 1;
    }
    if (done + (rows - r) > total) return 9;
    memcpy(peaks.data() + done * nbins, part.data() + r * nbins, (rows - r) * nbins * sizeof(HOST_F));
    done += rows - r;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) return 10;
  memcpy(peaks.data() + total * nbins, state.data(), nbins * sizeof(HOST_F));

  f = fopen(argv[9], "wb"); fwrite(peaks.data(), sizeof(HOST_F), (total + 1) * nbins, f); fclose(f);
  printf("CPP-SMOOTH-PEAK ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
