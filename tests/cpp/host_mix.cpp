// host_mix.cpp -- a C++ host's mix call through sdft::SDFT<T, F> (include/sdft/sdft.hpp): set_mix, mix_outputs and mix.  The
// facade's plans have one channel, so the mix has the one element {0}.  The checks are the host's own:
//   with the weight (0, 1) the rows are i times the rows of sdft_every(): (re, im) -> (-im, re), as numbers;
//   a mix with channel 1 is refused and leaves the mix alone; a call without a mix throws.
// Built and run by tests/test_gpu_mix.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp.
//
// usage: host_mix <dftsize> <x.raw>

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
  if (m != dftsize || sdft.mix_outputs() != 0) return 4;

  const size_t rows = (n - first + every - 1) / every;
  std::vector<std::complex<HOST_F>> want(rows * m), got(rows * m);
  if (sdft.sdft_every(n, x.data(), every, first, want.data()) != rows) return 5;

  bool thrown = false;
  try { sdft.mix(n, x.data(), every, first, 0, m, got.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_mix_n") != nullptr; }
  if (!thrown) return 6;

  const std::vector<std::complex<HOST_F>> w(m, std::complex<HOST_F>(0, 1));
  sdft.set_mix(1, 1, w.data());                              // the channels 0 ... 0
  if (sdft.mix_outputs() != 1) return 7;
  const size_t one[1] = {1};
  thrown = false;
  try { sdft.set_mix(1, 1, w.data(), one); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_set_mix") != nullptr; }
  if (!thrown || sdft.mix_outputs() != 1) return 8;

  sdft.reset();
  if (sdft.mix(n, x.data(), every, first, 0, m, got.data()) != rows) return 9;
  for (size_t i = 0; i < rows * m; ++i)
    if (got[i].real() != -want[i].imag() || got[i].imag() != want[i].real()) return 10;

  sdft.set_mix(0, 0, nullptr);
  if (sdft.mix_outputs() != 0) return 11;

  printf("CPP-MIX ok n=%zu m=%zu rows=%zu\n", n, m, rows);
  return 0;
}
