// smooth_peak_logic_test.cpp -- the host-side decisions of the smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the peak-hold call's for the same query), the refusals and
// their order, the grid of the carry pass (no row kept), and the whole scheme (smooth_peak_scheme: carry pass from +0, scan of the
// end values, row pass from S_c, hold over the windows) against the sequential loop and the exact recursion over a 40 dB burst:
// the loop's bits for one chunk and for decay 0, the hold of the scheme's own sequence whatever the grid, and the header's bound
// for several chunks.  Prints the largest ratio of an error to u M / (1 - a).
// Compiled by tests/test_smooth_peak_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.

#include "sdft_plan_logic.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

using namespace sdfthip::logic;

static int failures = 0;
#define CHECK(cond, ...)                                                                    \
  do {                                                                                      \
    if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
      if (failures > 20) exit(1); }                                                         \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static size_t rnd_in(size_t lo, size_t hi) { return lo + (size_t)(rnd() % (unsigned long long)(hi - lo + 1)); }
template <typename T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

static void test_route()
{
  CHECK(FK_SMOOTH_PEAK == 17, "get_option(\"last_kernel\") answers 17");
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery fq;
    fq.n = rnd_in(1, 2000000); fq.nbins = rnd_in(1, 4200); fq.channels = rnd_in(1, 8);
    const bool f32 = rnd() & 1;
    fq.fd_bytes = f32 ? 4 : 8; fq.fdx_bytes = f32 ? 8 : 16;
    fq.window = (int)rnd_in(0, 3); fq.cursor = rnd_in(0, 2 * fq.nbins - 1); fq.exact = f32 || (rnd() & 1); fq.fid_canonical = rnd() & 1;
    fq.analysis_batch = rnd() & 1; fq.pipe_wanted = rnd() & 1;
    if (rnd() % 4 == 0) fq.chunk = (long)rnd_in(1, 5000);
    if (rnd() % 4 == 0) fq.segments = (long)rnd_in(0, 4);
    if (rnd() % 4 == 0) fq.chain = (long)rnd_in(0, 2);
    fq.smooth_peak = true;
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_SMOOTH_PEAK, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    if (!fq.chunk && fq.n < 512) CHECK(r.chunks == 1, "n %zu: a call shorter than 512 samples is one chunk", fq.n);
    // the peak-hold and the smoothed power call of the same query: the same route in everything but the kernel
    for (int twin = 0; twin < 2; ++twin)
    {
      ForwardQuery pq = fq; pq.smooth_peak = false; (twin ? pq.power_smooth : pq.power_peak) = true;
      const ForwardRoute rp = forward_route(pq, [] { return true; });
      CHECK(rp.kernel == (twin ? FK_POWER_SMOOTH : FK_POWER_PEAK), "the twin's kernel");
      CHECK(rp.chunks == r.chunks && rp.len == r.len && rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums &&
            rp.relay_L == r.relay_L && rp.shift == r.shift && rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed &&
            rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map, "n %zu N %zu: not the twin's route", fq.n, fq.nbins);
    }
    // the carry pass keeps no row: forward_power_smooth_kernel stores a row only for a grid point below n
    const SmoothPeakCarryGrid g = smooth_peak_carry_grid(fq.n);
    CHECK(g.every >= 1 && every_rows(fq.n, g.every, g.first) == 0 && g.first >= fq.n, "n %zu: the carry pass's grid keeps a row", fq.n);
    CHECK(chunk_end(r.chunks - 1, r.len, r.shift, fq.n) == fq.n, "the last chunk ends the call");
  }
}

static void test_refusals()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int hold : {kHoldMax, kHoldMin})
    for (double ok : {0.0, 0.5, 1.0 - ldexp(1.0, -10)})
      CHECK(!smooth_peak_refusal<float>(hold, ok) && !smooth_peak_refusal<double>(hold, ok), "hold %d decay %g is accepted", hold, ok);
  for (int hold : {2, -1, 7})
  {
    const char* r = smooth_peak_refusal<double>(hold, 0.5);
    CHECK(r && strstr(r, "hold"), "hold %d is refused by name", hold);
    r = smooth_peak_refusal<double>(hold, nan);
    CHECK(r && strstr(r, "hold"), "the hold is named first");
  }
  for (double bad : {nan, -0.25, 1.0, 2.0})
  {
    const char* r = smooth_peak_refusal<float>(kHoldMin, bad);
    CHECK(r && strstr(r, "decay"), "decay %g is refused by name", bad);
  }
  const double near = 1.0 - ldexp(1.0, -26);
  CHECK(smooth_peak_refusal<float>(kHoldMax, near) && !smooth_peak_refusal<double>(kHoldMax, near), "1 - 2^-26: refused for FD float only");
}

// rows of the peak-hold grid over a sequence, by the rule
template <typename S> static std::vector<S> held(const std::vector<S>& s, size_t every, size_t first, int hold)
{
  const size_t n = s.size();
  std::vector<S> rows(power_sum_rows(n, every, first));
  for (size_t r = 0; r < rows.size(); ++r)
  {
    const size_t b = first > 0 ? (r == 0 ? 0 : first + (r - 1) * every) : r * every;
    const size_t e = std::min(n, first > 0 && r == 0 ? first : b + every);
    S m = s[b];
    for (size_t t = b + 1; t < e; ++t) m = peak_hold(m, s[t], hold);
    rows[r] = m;
  }
  return rows;
}

template <typename T> static long double test_scheme(const char* name)
{
  const long double u = ldexpl(1.0L, -std::numeric_limits<T>::digits);
  long double worst = 0;
  for (double decay : {0.0, 0.5, 0.9, 1.0 - ldexp(1.0, -10)})
  {
    const T a = (T)decay, b = (T)1 - a;
    for (int trial = 0; trial < 6; ++trial)
    {
      const size_t n = trial == 0 ? 300 : rnd_in(600, 4096);
      std::vector<T> p(n);
      for (size_t t = 0; t < n; ++t) p[t] = (T)((double)(rnd() % 1000003ull) / 1000003.0 * ((t / 500) % 3 == 1 ? 1e4 : 1.0));      // a 40 dB burst
      const T state = trial % 2 ? (T)3.25 : (T)0;
      // the sequential loop in T, and the exact recursion on the same terms and coefficients with its running largest value
      std::vector<T> seq(n);
      std::vector<long double> exact(n), big(n);
      volatile T s = state;
      long double x = state, m = state;
      for (size_t t = 0; t < n; ++t)
      {
        volatile T as = a * s, bp = b * p[t];
        s = as + bp; seq[t] = s;
        x = (long double)a * x + (long double)b * (long double)p[t]; exact[t] = x;
        m = std::max(m, x); big[t] = m;
      }
      std::vector<T> own(n);
      T end = smooth_peak_scheme<T>(p.data(), n, a, state, (long)n, 0, own.data());
      CHECK(memcmp(own.data(), seq.data(), n * sizeof(T)) == 0 && same_bits(end, seq[n - 1]), "%s decay %g: one chunk is the sequential loop", name, decay);
      for (long len : {64L, 512L, 333L})
        for (long shift : {0L, 17L})
        {
          end = smooth_peak_scheme<T>(p.data(), n, a, state, len, shift, own.data());
          CHECK(same_bits(end, own[n - 1]), "%s: the state is the last value of the row pass", name);
          if (a == (T)0) { CHECK(memcmp(own.data(), seq.data(), n * sizeof(T)) == 0, "%s: decay 0 has the loop's bits in any chunking", name); continue; }
          const long double unit = u / (1.0L - (long double)a);
          for (size_t t = 0; t < n; ++t)
          {
            const long double err = fabsl((long double)own[t] - exact[t]);
            worst = std::max(worst, err / (unit * big[t]));
            if (err > 8 * unit * big[t]) { CHECK(false, "%s decay %g len %ld shift %ld sample %zu: %Lg beyond %Lg", name, decay, len, shift, t, err, 8 * unit * big[t]); break; }
          }
          // the hold: |ext(x') - ext(x)| <= max |x' - x| over the window, which M at the window's end bounds
          for (int hold : {kHoldMax, kHoldMin})
          {
            const size_t every = rnd_in(1, 700), first = rnd_in(0, 800);
            const std::vector<T> got = held(own, every, first, hold);
            const std::vector<long double> want = held(exact, every, first, hold), top = held(big, every, first, kHoldMax);
            for (size_t r = 0; r < got.size(); ++r)
            {
              const long double err = fabsl((long double)got[r] - want[r]);
              worst = std::max(worst, err / (unit * top[r]));
              if (err > 8 * unit * top[r]) { CHECK(false, "%s decay %g len %ld every %zu first %zu row %zu: %Lg beyond the bound", name, decay, len, every, first, r, err); break; }
            }
          }
        }
    }
  }
  printf("%s: largest error of the scheme %.3Lf u M / (1 - a)\n", name, worst);
  return worst;
}

int main()
{
  test_route();
  test_refusals();
  const long double wf = test_scheme<float>("float"), wd = test_scheme<double>("double");
  printf("worst ratio to u M / (1 - a): %.2Lf\n", std::max(wf, wd));
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("smooth-peak-logic: all properties hold\n");
  return 0;
}
