// host_power_moments.cpp -- a C++ host's power-moments calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): a stream in blocks of
// `block` samples on the grid of `every` samples, head rows added, both components, to the rows they complete.  The host's own
// checks:
//   the first component of a call is power_sum's row of a twin plan bit for bit;
//   a band past the last bin throws, with the call's name in the text.
// Built and run by tests/test_gpu_power_moments.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp; the test compares
// the file with the Python call's bits.
//
// usage: host_power_moments <dftsize> <every> <block> <bin0> <nbins> <x.raw> <moments.raw>

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
  if (argc < 8) return 2;
  const size_t dftsize = (size_t)atol(argv[1]), every = (size_t)atol(argv[2]), block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]), nbins = (size_t)atol(argv[5]), pair = 2 * nbins;

  FILE* f = fopen(argv[6], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / sizeof(HOST_T);
  fseek(f, 0, SEEK_SET);
  std::vector<HOST_T> x(n);
  if (fread(x.data(), sizeof(HOST_T), n, f) != n) return 3;
  fclose(f);

  SDFT<HOST_T, HOST_F> sdft(dftsize, sdft::Window::Hann, 1), twin(dftsize, sdft::Window::Hann, 1);
  if (sdft.size() != dftsize) return 4;

  const size_t total = (n + every - 1) / every;
  std::vector<HOST_F> moments(total * pair), part((block / every + 2) * pair), sums((block / every + 2) * nbins);

  bool thrown = false;
  try { sdft.power_moments(block, x.data(), every, 0, dftsize, 1, part.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_power_moments_n") != nullptr; }
  if (!thrown) return 5;

  size_t done = 0, first = 0, calls = 0;
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t rows = sdft.power_moments(m, x.data() + t, every, first, bin0, nbins, part.data());
    if (rows == 0 || twin.power_sum(m, x.data() + t, every, first, bin0, nbins, sums.data()) != rows) return 6;
    for (size_t i = 0; i < rows * nbins; ++i)
      if (memcmp(&part[2 * i], &sums[i], sizeof(HOST_F)) != 0) { fprintf(stderr, "call %zu element %zu\n", calls, i); return 7; }
    size_t r = 0;
    if (first > 0)
    {
      if (done == 0) return 8;
      for (size_t k = 0; k < pair; ++k) moments[(done - 1) * pair + k] = moments[(done - 1) * pair + k] + part[k];
      r = 1;
    }
    if (done + (rows - r) > total) return 9;
    memcpy(moments.data() + done * pair, part.data() + r * pair, (rows - r) * pair * sizeof(HOST_F));
    done += rows - r;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) return 10;

  f = fopen(argv[7], "wb"); fwrite(moments.data(), sizeof(HOST_F), total * pair, f); fclose(f);
  printf("CPP-POWER-MOMENTS ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
