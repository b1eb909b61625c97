// host_power_smooth.cpp -- a C++ host's smoothed power calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): a stream in blocks of
// `block` samples on the grid of `every` samples, the average passed from call to call in `state`.  The host's own checks:
//   decay 0 on a twin plan is power()'s rows bit for bit;
//   a decay of 1 throws, with the call's name in the text, and leaves state alone.
// Built and run by tests/test_gpu_power_smooth.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp; the test compares
// the file -- the rows, then the state after the last sample -- with the sequential recursion over the oracle's powers.
//
// usage: host_power_smooth <dftsize> <every> <block> <bin0> <nbins> <decay> <x.raw> <smooth.raw>

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
  if (argc < 9) return 2;
  const size_t dftsize = (size_t)atol(argv[1]), every = (size_t)atol(argv[2]), block = (size_t)atol(argv[3]);
  const size_t bin0 = (size_t)atol(argv[4]), nbins = (size_t)atol(argv[5]);
  const double decay = atof(argv[6]);

  FILE* f = fopen(argv[7], "rb");
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
  std::vector<HOST_F> smooth((total + 1) * nbins), state(nbins, (HOST_F)0), a((block / every + 2) * nbins), b((block / every + 2) * nbins);

  bool thrown = false;
  state[0] = (HOST_F)7;
  try { sdft.power_smooth(block, x.data(), every, 0, bin0, nbins, 1.0, state.data(), smooth.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_power_smooth_n") != nullptr; }
  if (!thrown || state[0] != (HOST_F)7) return 5;
  state[0] = (HOST_F)0;

  size_t done = 0, first = 0, calls = 0;
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    if (done + grid > total) return 9;
    if (sdft.power_smooth(m, x.data() + t, every, first, bin0, nbins, decay, state.data(), grid ? smooth.data() + done * nbins : nullptr) != grid) return 6;
    // decay 0 forgets at once: power()'s rows, bit for bit, with or without a state
    if (zero.power_smooth(m, x.data() + t, every, first, bin0, nbins, 0.0, nullptr, a.data()) != grid ||
        twin.power(m, x.data() + t, every, first, bin0, nbins, b.data()) != grid) return 7;
    if (memcmp(a.data(), b.data(), grid * nbins * sizeof(HOST_F)) != 0) { fprintf(stderr, "call %zu: decay 0 is not power()\n", calls); return 8; }
    done += grid;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) return 10;
  memcpy(smooth.data() + total * nbins, state.data(), nbins * sizeof(HOST_F));

  f = fopen(argv[8], "wb"); fwrite(smooth.data(), sizeof(HOST_F), (total + 1) * nbins, f); fclose(f);
  printf("CPP-POWER-SMOOTH ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
