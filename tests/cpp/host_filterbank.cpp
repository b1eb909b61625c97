// host_filterbank.cpp -- a C++ host's filterbank and pooled-power calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp):
// set_filterbank, filterbank_bands, filterbank and power_sum.  The checks are the host's own:
//   a whole-row band of weight 1 is, row by row, the sum over the bins of power_sum's every == 1 rows (the powers themselves), within
//   the contract's bar for a band of L = dftsize bins -- FD float gamma_(L+1) T + L eta against the sum in double, FD double
//   2 gamma_L T + L eta, the host's double sum erring by up to gamma_L T itself;
//   dftsize one-bin bands of weight 1 are those rows bit for bit;
//   a call without a filterbank throws.
// Built and run by tests/test_gpu_filterbank.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp.
//
// usage: host_filterbank <dftsize> <x.raw>

#include <sdft/sdft.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
  if (argc < 3) return 2;
  const size_t dftsize = (size_t)atol(argv[1]);

  FILE* f = fopen(argv[2], "rb");
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

  // the powers of every row: windows of one sample
  std::vector<HOST_F> p(n * m);
  if (sdft.power_sum(n, x.data(), 1, 0, 0, m, p.data()) != n) return 5;

  // one band over the whole row
  const std::vector<HOST_F> ones(m, (HOST_F)1);
  const size_t row_bin0 = 0, row_nbins = m;
  sdft.set_filterbank(1, &row_bin0, &row_nbins, ones.data());
  if (sdft.filterbank_bands() != 1) return 6;
  std::vector<HOST_F> whole(n);
  sdft.reset();
  if (sdft.filterbank(n, x.data(), 1, 0, whole.data()) != n) return 7;
  const bool single = sizeof(HOST_F) == 4;
  const double u = (double)std::numeric_limits<HOST_F>::epsilon() / 2, eta = (double)std::numeric_limits<HOST_F>::denorm_min();
  const double terms = single ? (double)(m + 1) : (double)m;
  const double gamma = (single ? 1.0 : 2.0) * terms * u / (1.0 - terms * u);
  double worst = 0;
  for (size_t r = 0; r < n; ++r)
  {
    double T = 0;                                                // (powers: T = sum |w p| is the sum itself)
    for (size_t k = 0; k < m; ++k) T += (double)p[r * m + k];
    const double err = std::fabs((double)whole[r] - T), bar = gamma * T + (double)m * eta;
    if (!(err <= bar)) { fprintf(stderr, "row %zu: %g against %g, error %g, bar %g\n", r, (double)whole[r], T, err, bar); return 8; }
    if (bar > 0 && err / bar > worst) worst = err / bar;
  }

  // one band per bin
  std::vector<size_t> bin0(m), nbins(m, 1);
  for (size_t k = 0; k < m; ++k) bin0[k] = k;
  sdft.set_filterbank(m, bin0.data(), nbins.data(), ones.data());
  if (sdft.filterbank_bands() != m) return 9;
  std::vector<HOST_F> each(n * m);
  sdft.reset();
  if (sdft.filterbank(n, x.data(), 1, 0, each.data()) != n) return 10;
  if (memcmp(each.data(), p.data(), n * m * sizeof(HOST_F)) != 0) return 11;

  // no bands: the filterbank is removed, and the call says so
  sdft.set_filterbank(0, nullptr, nullptr, nullptr);
  if (sdft.filterbank_bands() != 0) return 12;
  bool thrown = false;
  try { sdft.filterbank(n, x.data(), 1, 0, each.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_filterbank_n") != nullptr; }
  if (!thrown) return 13;

  printf("CPP-FILTERBANK ok n=%zu m=%zu largest error / bar = %.3g\n", n, m, worst);
  return 0;
}
