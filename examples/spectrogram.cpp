// spectrogram.cpp -- C++ host in the shape of the reference's cpp/examples/analysis.cpp (without the
// plotting): sdft::SDFT<float, double> over a chirp, prints the strongest bin every 4000 samples.  Only those rows are
// formed, only as powers and only for the band the sweep crosses (power: 12 rows of 520 real numbers instead of the
// 48000 x 1000 complex matrix).  With the argument `pooled` a row is not the power AT every 4000th sample but the mean of the
// power over the 4000 samples up to it (power_sum: the sums of the windows, divided by their length here).
//
//   make -C examples && ./examples/spectrogram [pooled]

#include <sdft/sdft.h>      // resolves to include/cpp/sdft/sdft.h -> sdft/sdft.hpp

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char* argv[])
{
  const bool pooled = argc > 1 && !std::strcmp(argv[1], "pooled");
  const size_t sr = 48000, n = 48000, m = 1000;
  std::vector<float> x(n);
  double phi = 0;
  for (size_t i = 0; i < n; ++i)
  {
    const double f = (double)i / n * sr / 4;            // 0 -> 12 kHz
    phi += 2.0 * 3.14159265358979323846 * f / sr;
    x[i] = (float)std::sin(phi);
  }
  sdft::SDFT<float, double> sdft(m, sdft::Window::Hann, 1);
  const size_t first = 3999, every = 4000;
  const size_t bin0 = 0, nbins = 520;                   // 0 ... 12.5 kHz: bin k is k * sr / (2 m) Hz
  std::vector<double> power(((n - first + every - 1) / every + 1) * nbins);
  // pooled: the grid is moved by one sample so that its windows END with the samples the other form looks at -- here to 0:
  // window r is [r * every, (r + 1) * every), its last sample first + r * every, and every window is whole (every divides n)
  const size_t rows = pooled ? sdft.power_sum(n, x.data(), every, (first + 1) % every, bin0, nbins, power.data())
                             : sdft.power(n, x.data(), every, first, bin0, nbins, power.data());
  for (size_t r = 0; r < rows; ++r)
  {
    const size_t t = first + r * every;
    double* row = power.data() + r * nbins;
    if (pooled)
      for (size_t k = 0; k < nbins; ++k) row[k] /= (double)every;     // sums -> means (every window is whole here)
    size_t best = 0;
    for (size_t k = 1; k < nbins; ++k)
      if (row[k] > row[best]) best = k;
    best += bin0;
    std::printf("t=%6zu  peak bin %4zu  ~%7.1f Hz  (instantaneous sweep frequency %7.1f Hz, window centre ~%zu samples earlier)\n",
                t, best, (double)best * sr / (2.0 * m), (double)t / n * sr / 4, m);
  }
  return 0;
}
