// host_cross_smooth.cpp -- a C++ host's smoothed cross-spectrum calls through sdft::SDFT<T, F> (include/sdft/sdft.hpp): a stream in
// blocks of `block` samples on the grid of `every` samples, the average of the pair (0, 0) -- twice in the list -- passed from call to
// call in `state`.  The host's own checks:
//   the real part of the pair (0, 0) is power_smooth()'s value on a twin plan bit for bit, its imaginary part is +0;
//   the repeated pair has the first one's bits;
//   decay 0 on a third plan is cross_sum()'s every == 1 term at the grid's samples;
//   a decay of 1 throws, with the call's name in the text, and leaves state alone; so does a plan without pairs.
// Built and run by tests/test_gpu_cross_smooth.py with g++ -std=c++11 -DHOST_T=... -DHOST_F=... -Iinclude/cpp; the test compares
// the file -- the rows of pair 0, then its state after the last sample -- with the sequential recursion over the oracle's rows.
//
// usage: host_cross_smooth <dftsize> <every> <block> <bin0> <nbins> <decay> <x.raw> <smooth.raw>

#include <sdft/sdft.h>

#include <cmath>
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
typedef std::complex<HOST_F> cplx;

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

  SDFT<HOST_T, HOST_F> sdft(dftsize, sdft::Window::Hann, 1), zero(dftsize, sdft::Window::Hann, 1), twin(dftsize, sdft::Window::Hann, 1),
      sums(dftsize, sdft::Window::Hann, 1);
  if (sdft.size() != dftsize) return 4;

  const size_t total = (n + every - 1) / every, most = block / every + 2;
  std::vector<cplx> smooth((total + 1) * nbins), state(2 * nbins, cplx(0, 0)), piece(2 * most * nbins), term(block * nbins), a(most * nbins);
  std::vector<HOST_F> power(most * nbins), pstate(nbins, (HOST_F)0);

  bool thrown = false;
  try { sdft.cross_smooth(block, x.data(), every, 0, bin0, nbins, decay, state.data(), piece.data()); }      // no pairs yet
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_cross_smooth_n") != nullptr; }
  if (!thrown) return 5;
  const size_t pa[2] = {0, 0}, pb[2] = {0, 0};
  sdft.set_pairs(2, pa, pb); zero.set_pairs(1, pa, pb); sums.set_pairs(1, pa, pb);
  thrown = false;
  state[0] = cplx(7, 0);
  try { sdft.cross_smooth(block, x.data(), every, 0, bin0, nbins, 1.0, state.data(), piece.data()); }
  catch (const std::runtime_error& e) { thrown = strstr(e.what(), "sdft_hip_sdft_cross_smooth_n") != nullptr; }
  if (!thrown || state[0] != cplx(7, 0)) return 5;
  state[0] = cplx(0, 0);

  size_t done = 0, first = 0, calls = 0;
  for (size_t t = 0; t < n; t += block, ++calls)
  {
    const size_t m = n - t < block ? n - t : block;
    const size_t grid = first < m ? (m - first - 1) / every + 1 : 0;
    if (done + grid > total || grid > most) return 9;
    if (sdft.cross_smooth(m, x.data() + t, every, first, bin0, nbins, decay, state.data(), grid ? piece.data() : nullptr) != grid) return 6;
    if (twin.power_smooth(m, x.data() + t, every, first, bin0, nbins, decay, pstate.data(), grid ? power.data() : nullptr) != grid) return 6;
    for (size_t i = 0; i < grid * nbins; ++i)
    {
      const HOST_F re = piece[i].real(), im = piece[i].imag();
      if (memcmp(&re, &power[i], sizeof(HOST_F)) != 0 || im != (HOST_F)0 || std::signbit(im)) { fprintf(stderr, "call %zu: pair (0, 0) is not power_smooth()\n", calls); return 7; }
    }
    if (memcmp(piece.data(), piece.data() + grid * nbins, grid * nbins * sizeof(cplx)) != 0) { fprintf(stderr, "call %zu: the repeated pair differs\n", calls); return 7; }
    // decay 0 forgets at once: the cross-spectrum call's every == 1 term at the grid's samples
    if (zero.cross_smooth(m, x.data() + t, every, first, bin0, nbins, 0.0, nullptr, a.data()) != grid ||
        sums.cross_sum(m, x.data() + t, 1, 0, bin0, nbins, term.data()) != m) return 7;
    for (size_t r = 0; r < grid; ++r)
      for (size_t k = 0; k < nbins; ++k)
        if (a[r * nbins + k] != term[(first + r * every) * nbins + k]) { fprintf(stderr, "call %zu: decay 0 is not the term\n", calls); return 8; }
    memcpy(smooth.data() + done * nbins, piece.data(), grid * nbins * sizeof(cplx));
    done += grid;
    first = grid ? first + grid * every - m : first - m;
  }
  if (done != total) return 10;
  memcpy(smooth.data() + total * nbins, state.data(), nbins * sizeof(cplx));
  for (size_t k = 0; k < nbins; ++k)
    if (state[k].real() != pstate[k] || state[k] != state[nbins + k]) return 11;

  f = fopen(argv[8], "wb"); fwrite(smooth.data(), sizeof(cplx), (total + 1) * nbins, f); fclose(f);
  printf("CPP-CROSS-SMOOTH ok n=%zu rows=%zu calls=%zu\n", n, total, calls);
  return 0;
}
