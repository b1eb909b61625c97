// host_covariance.cpp -- a C++ host's covariance call through sdft::SDFT<T, F> (include/sdft/sdft.hpp): set_array, array_channels and
// covariance.  The facade's plans have one channel, so the array is {0} and the matrix is 1 x 1: the auto-spectrum.  The checks are
// the host's own:
//   the one element is cross_sum's pair (0, 0) bit for bit;
//   a list with channel 1 is refused and leaves the array alone; a call without an array throws.
// Built and run by tests/test_gpu_covariance.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp.
//
// usage: host_covariance <dftsize> <x.raw>

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
  const size_t m = sdft.size(), every = 100, first = 37;
  if (m != dftsize || sdft.array_channels() != 0) return 4;

  const size_t zero[1] = {0}, one[1] = {1};
  sdft.set_pairs(1, zero, zero);
  const size_t rows = (n - first + every - 1) / every + 1;
  std::vector<std::complex<HOST_F>> want(rows * m), got(rows * m);
  if (sdft.cross_sum(n, x.data(), every, first, 0, m, want.data()) != rows) return 5;

  bool thrown = false;
  try { sdft.covariance(n, x.data(), every, first, 0, m, got.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_covariance_n") != nullptr; }
  if (!thrown) return 6;

  sdft.set_array(1);                                        // the channels 0 ... 0
  if (sdft.array_channels() != 1) return 7;
  thrown = false;
  try { sdft.set_array(1, one); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_set_array") != nullptr; }
  if (!thrown || sdft.array_channels() != 1 || sdft.pairs() != 1) return 8;
  sdft.set_array(1, zero);

  sdft.reset();
  if (sdft.covariance(n, x.data(), every, first, 0, m, got.data()) != rows) return 9;
  if (memcmp(got.data(), want.data(), rows * m * sizeof(std::complex<HOST_F>)) != 0) return 10;

  sdft.set_array(0);
  if (sdft.array_channels() != 0 || sdft.pairs() != 1) return 11;

  printf("CPP-COVARIANCE ok n=%zu m=%zu rows=%zu\n", n, m, rows);
  return 0;
}
