// spectrogram.cpp -- C++ host in the shape of the reference's cpp/examples/analysis.cpp (without the
// plotting): sdft::SDFT<float, double> over a chirp, prints the strongest bin every 4000 samples.  Only those rows are
// formed, only as powers and only for the band the sweep crosses (power: 12 rows of 520 real numbers instead of the
// 48000 x 1000 complex matrix).
//
//   make -C examples && ./examples/spectrogram

#include <sdft/sdft.h>      // resolves to include/cpp/sdft/sdft.h -> sdft/sdft.hpp

#include <cmath>
#include <cstdio>
#include <vector>

int main()
{
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
  std::vector<double> power((n - first + every - 1) / every * nbins);
  const size_t rows = sdft.power(n, x.data(), every, first, bin0, nbins, power.data());
  for (size_t r = 0; r < rows; ++r)
  {
    const size_t t = first + r * every;
    const double* row = power.data() + r * nbins;
    size_t best = 0;
    for (size_t k = 1; k < nbins; ++k)
      if (row[k] > row[best]) best = k;
    best += bin0;
    std::printf("t=%6zu  peak bin %4zu  ~%7.1f Hz  (instantaneous sweep frequency %7.1f Hz, window centre ~%zu samples earlier)\n",
                t, best, (double)best * sr / (2.0 * m), (double)t / n * sr / 4, m);
  }
  return 0;
}
