// cross_smooth_logic_test.cpp -- the host-side decisions of the smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the cross-spectrum call's for the same items), the unit row,
// the workspace and its slots with pairs for channels, that item i < npairs is unit i, the decay check -- then the whole scheme
// (local scans from +0, scan of the end values, fix-up, each on the 2 * nbins real numbers of a pair) on SIGNED terms against the
// sequential loop: the bits of it for one chunk and for decay 0, within the header's bound 8 u M / (1 - a) for several chunks,
// M the running largest of the majorant m = a m + b |term| started at |state|.
// Compiled by tests/test_cross_smooth_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
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
static double rnd_signed() { return (double)(rnd() % 2000003ull) / 1000001.0 - 1.0; }      // [-1, 1]
template <typename T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

static void test_route()
{
  CHECK(FK_CROSS_SMOOTH == 16, "get_option(\"last_kernel\") answers 16");
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
    fq.cross_smooth = true; fq.cross_items = rnd_in(1, 40);
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_CROSS_SMOOTH, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    if (!fq.chunk && fq.n < 512) CHECK(r.chunks == 1, "n %zu: a call shorter than 512 samples is one chunk", fq.n);
    // the cross-spectrum call of the same items: the same route in everything but the kernel
    ForwardQuery cq = fq; cq.cross_smooth = false; cq.cross_sum = true;
    const ForwardRoute rc = forward_route(cq, [] { return true; });
    CHECK(rc.kernel == FK_CROSS_SUM, "the cross-spectrum call's kernel");
    CHECK(rc.chunks == r.chunks && rc.len == r.len && rc.tiles == r.tiles && rc.interior == r.interior && rc.carry == r.carry && rc.sums == r.sums &&
          rc.relay_L == r.relay_L && rc.shift == r.shift && rc.segments == r.segments && rc.delta_in_carry == r.delta_in_carry && rc.use_seed == r.use_seed &&
          rc.vec_store == r.vec_store && rc.xcd_map == r.xcd_map, "n %zu N %zu: not the cross-spectrum call's route", fq.n, fq.nbins);
    for (long c = 0; c < r.chunks; c += std::max(1L, r.chunks / 7))
    {
      const size_t t0 = chunk_begin(c, r.len, r.shift), t1 = chunk_end(c, r.len, r.shift, fq.n);
      CHECK(t0 < t1 && t1 - t0 <= (size_t)r.len, "n %zu chunk %ld of %ld: [%zu, %zu) of len %ld", fq.n, c, r.chunks, t0, t1, r.len);
    }
    CHECK(chunk_end(r.chunks - 1, r.len, r.shift, fq.n) == fq.n, "the last chunk ends the call");
  }
}

static void test_sizes()
{
  CHECK(cross_smooth_unit_row(1) == 2 && cross_smooth_unit_row(1024) == 2048, "a unit row is (re, im) of every bin of the band");
  CHECK(power_smooth_workspace(3, 1, cross_smooth_unit_row(100)) == 0, "a call of one chunk has no workspace");
  for (int i = 0; i < 2000; ++i)
  {
    const size_t npairs = rnd_in(1, 9), chunks = rnd_in(2, 40), nb = rnd_in(1, 300), row = cross_smooth_unit_row(nb);
    CHECK(power_smooth_workspace(npairs, chunks, row) == npairs * chunks * 2 * nb, "size");
    size_t expect = 0;
    bool dense = true;
    for (size_t p = 0; p < npairs; ++p)
      for (size_t j = 0; j < chunks; ++j, expect += row) dense = dense && power_smooth_slot(p, chunks, j, row) == expect;
    CHECK(dense && expect == power_smooth_workspace(npairs, chunks, row), "slots tile the workspace");
    // the complex slot of bin k of (pair, chunk) in the kernel's eyes is the real slots 2k, 2k + 1 in the carry kernels'
    const size_t p = rnd_in(0, npairs - 1), j = rnd_in(0, chunks - 1), k = rnd_in(0, nb - 1);
    CHECK((p * chunks + j) * 2 * nb + 2 * k == power_smooth_slot(p, chunks, j, row) + 2 * k, "the interleaved slot");
  }
  // item i < npairs is unit i, whatever the list: repeats, a == b, channels in no pair
  for (int i = 0; i < 500; ++i)
  {
    const size_t channels = rnd_in(1, 7), npairs = rnd_in(1, 12);
    std::vector<size_t> a(npairs), b(npairs);
    for (size_t p = 0; p < npairs; ++p) { a[p] = rnd_in(0, channels - 1); b[p] = rnd_in(0, channels - 1); }
    const std::vector<CrossItem> items = cross_items(channels, npairs, a.data(), b.data());
    CHECK(items.size() >= npairs, "an item per pair");
    std::vector<int> writers(channels, 0);
    for (size_t p = 0; p < items.size(); ++p)
    {
      if (p < npairs) CHECK(items[p].out == (int)p && items[p].a == a[p] && items[p].b == b[p], "item %zu is pair %zu", p, p);
      else CHECK(items[p].out < 0 && items[p].a == items[p].b, "the items after the pairs only advance a channel");
      if (items[p].writes_a) ++writers[items[p].a];
      if (items[p].writes_b && items[p].a != items[p].b) ++writers[items[p].b];
    }
    for (size_t c = 0; c < channels; ++c) CHECK(writers[c] == 1, "channel %zu has %d writers", c, writers[c]);
  }
}

static void test_decay()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double ok : {0.0, 0.5, 0.9, 1.0 - ldexp(1.0, -10), -0.0})
    CHECK(power_smooth_decay_ok<float>(ok) && power_smooth_decay_ok<double>(ok), "decay %.17g is accepted", ok);
  for (double bad : {nan, inf, -inf, 1.0, 1.5, -1e-30, -0.5})
    CHECK(!power_smooth_decay_ok<float>(bad) && !power_smooth_decay_ok<double>(bad), "decay %.17g is refused", bad);
  const double near = 1.0 - ldexp(1.0, -26);
  CHECK(!power_smooth_decay_ok<float>(near) && power_smooth_decay_ok<double>(near), "1 - 2^-26: refused for FD float, accepted for FD double");
}

// the kernels' scheme on the host for ONE real number of a unit's row (the carry kernels are elementwise): chunk 0 from the state,
// later chunks from +0, the scan of the end values in ascending order, the fix-up of the rows of the later chunks
template <typename T> static void chunked(const std::vector<T>& p, T a, T state, long len, long shift, std::vector<T>& rows, T& end)
{
  const size_t n = p.size();
  const T b = (T)1 - a;
  const long chunks = (long)((n + (size_t)shift + (size_t)len - 1) / (size_t)len);
  const std::vector<T> pw = power_smooth_table<T>(a, (size_t)len);
  std::vector<T> ends((size_t)chunks);
  rows.assign(n, (T)0);
  for (long c = 0; c < chunks; ++c)
  {
    volatile T s = c ? (T)0 : state;
    for (size_t t = chunk_begin(c, len, shift); t < chunk_end(c, len, shift, n); ++t)
    {
      volatile T as = a * s, bp = b * p[t];
      s = as + bp;
      rows[t] = s;
    }
    ends[(size_t)c] = s;
  }
  if (chunks == 1) { end = ends[0]; return; }
  volatile T s = ends[0];
  for (long c = 1; c < chunks; ++c)
  {
    const T e = ends[(size_t)c];
    ends[(size_t)c] = s;
    volatile T ps = pw[chunk_end(c, len, shift, n) - chunk_begin(c, len, shift)] * s;
    s = ps + e;
  }
  end = s;
  for (size_t t = 0; t < n; ++t)
  {
    const PowerSmoothFix f = power_smooth_fix(t, len, shift);
    if (f.chunk == 0) continue;
    volatile T ps = pw[f.power] * ends[(size_t)f.chunk];
    rows[t] = rows[t] + ps;
  }
}

// signed, partly correlated terms with a 40 dB burst: re and im of A conj(B), B = 0.5 A + independent noise
template <typename T> static void signed_terms(size_t n, std::vector<T>& re, std::vector<T>& im)
{
  re.resize(n); im.resize(n);
  for (size_t t = 0; t < n; ++t)
  {
    const double g = (t / 500) % 3 == 1 ? 100.0 : 1.0;
    const T ar = (T)(g * rnd_signed()), ai = (T)(g * rnd_signed());
    const T br = (T)(0.5 * (double)ar + g * 0.7 * rnd_signed()), bi = (T)(0.5 * (double)ai + g * 0.7 * rnd_signed());
    volatile T rr = ar * br, ii = ai * bi, ir = ai * br, ri = ar * bi;
    re[t] = rr + ii; im[t] = ir - ri;
  }
}

template <typename T> static void test_scheme(const char* name)
{
  const long double u = ldexpl(1.0L, -std::numeric_limits<T>::digits);
  long double worst = 0;
  for (double decay : {0.0, 0.5, 0.9, 1.0 - ldexp(1.0, -10)})
  {
    const T a = (T)decay, b = (T)1 - a;
    for (int trial = 0; trial < 6; ++trial)
    {
      const size_t n = trial == 0 ? 300 : rnd_in(600, 4096);
      std::vector<T> comp[2];
      signed_terms<T>(n, comp[0], comp[1]);
      for (int k = 0; k < 2; ++k)
      {
        const std::vector<T>& p = comp[k];
        const T state = trial % 2 ? (T)(k ? -3.25 : 2.5) : (T)0;
        // the sequential loop in T, the exact recursion on the same terms and coefficients, and the majorant
        std::vector<T> seq(n);
        std::vector<long double> exact(n), big(n);
        volatile T s = state;
        long double x = state, m = fabsl((long double)state), top = m;
        for (size_t t = 0; t < n; ++t)
        {
          volatile T as = a * s, bp = b * p[t];
          s = as + bp; seq[t] = s;
          x = (long double)a * x + (long double)b * (long double)p[t]; exact[t] = x;
          m = (long double)a * m + (long double)b * fabsl((long double)p[t]);
          top = std::max(top, m); big[t] = top;
          CHECK(fabsl(x) <= m * (1 + 1e-15L), "|s| <= m");
        }
        std::vector<T> rows; T end;
        chunked(p, a, state, (long)n, 0, rows, end);
        CHECK(memcmp(rows.data(), seq.data(), n * sizeof(T)) == 0 && same_bits(end, seq[n - 1]), "%s decay %g: one chunk is the sequential loop", name, decay);
        for (long len : {40L, 64L, 512L, 333L})
          for (long shift : {0L, 17L})
          {
            chunked(p, a, state, len, shift, rows, end);
            if (a == (T)0)
            {
              // (+0 + x: a -0 term comes out as +0 -- equal as numbers)
              bool equal = end == seq[n - 1];
              for (size_t t = 0; t < n; ++t) equal = equal && rows[t] == seq[t];
              CHECK(equal, "%s: decay 0 has the loop's numbers in any chunking", name);
              continue;
            }
            for (size_t t = 0; t < n; ++t)
            {
              const long double unit = u * big[t] / (1.0L - (long double)a), err = fabsl((long double)rows[t] - exact[t]);
              if (unit > 0) worst = std::max(worst, err / unit);
              if (err > 8 * unit) { CHECK(false, "%s decay %g len %ld shift %ld sample %zu: %Lg beyond %Lg", name, decay, len, shift, t, err, 8 * unit); break; }
            }
            CHECK(fabsl((long double)end - exact[n - 1]) <= 8 * u * big[n - 1] / (1.0L - (long double)a), "%s: the end value", name);
          }
      }
    }
  }
  CHECK(worst <= 8, "%s: ratio %.3Lf", name, worst);
  printf("%s: largest chunked error on signed terms %.3Lf u M / (1 - a)\n", name, worst);
}

int main()
{
  test_route();
  test_sizes();
  test_decay();
  test_scheme<float>("float");
  test_scheme<double>("double");
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("cross-smooth-logic: all properties hold\n");
  return 0;
}
