// host_cross_sum.cpp -- a C++ host's cross-spectrum calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): set_pairs, pairs and
// cross_sum.  The facade's plans have one channel, so the list is the auto-spectrum (0, 0), once and repeated.  The checks are the
// host's own:
//   at every == 1 the real part is power_sum's every == 1 row bit for bit and the imaginary part is +0;
//   a repeated pair gives the same bits;
//   pair (0, 1) is refused and leaves the list alone; a call without pairs throws.
// Built and run by tests/test_gpu_cross_sum.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp.
//
// usage: host_cross_sum <dftsize> <x.raw>

#include <sdft/sdft.h>

#include <complex>
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
  if (m != dftsize || sdft.pairs() != 0) return 4;

  // the powers of every row: windows of one sample
  std::vector<HOST_F> p(n * m);
  if (sdft.power_sum(n, x.data(), 1, 0, 0, m, p.data()) != n) return 5;

  std::vector<std::complex<HOST_F>> s(2 * n * m);
  bool thrown = false;
  try { sdft.cross_sum(n, x.data(), 1, 0, 0, m, s.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_cross_sum_n") != nullptr; }
  if (!thrown) return 6;

  const size_t zeros[2] = {0, 0}, ones[2] = {1, 1};
  sdft.set_pairs(2, zeros, zeros);
  if (sdft.pairs() != 2) return 7;
  thrown = false;
  try { sdft.set_pairs(1, zeros, ones); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_set_pairs") != nullptr; }
  if (!thrown || sdft.pairs() != 2) return 8;

  sdft.reset();
  if (sdft.cross_sum(n, x.data(), 1, 0, 0, m, s.data()) != n) return 9;
  const HOST_F zero = 0;
  for (size_t i = 0; i < n * m; ++i)
  {
    const HOST_F re = s[i].real(), im = s[i].imag();
    if (memcmp(&re, &p[i], sizeof(HOST_F)) != 0 || memcmp(&im, &zero, sizeof(HOST_F)) != 0) { fprintf(stderr, "element %zu\n", i); return 10; }
  }
  if (memcmp(s.data(), s.data() + n * m, n * m * sizeof(std::complex<HOST_F>)) != 0) return 11;

  sdft.set_pairs(0, nullptr, nullptr);
  if (sdft.pairs() != 0) return 12;

  printf("CPP-CROSS-SUM ok n=%zu m=%zu\n", n, m);
  return 0;
}
