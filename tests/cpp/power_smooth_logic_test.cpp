// power_smooth_logic_test.cpp -- the host-side decisions of the smoothed power analysis (sdft_hip_sdft_power_smooth_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the pooled power call's for the same query), the rows (the
// power call's), the workspace and its slots, the decay check, the table of the decay's powers, and the chunk-and-offset rule of
// the fix-up against a walk over the chunks -- then the whole scheme (local scans from +0, scan of the end values, fix-up) against
// the sequential loop: the bits of it for one chunk and for decay 0, within the header's bound for several chunks.
// Compiled by tests/test_power_smooth_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
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
  CHECK(FK_POWER_SMOOTH == 15, "get_option(\"last_kernel\") answers 15");
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
    fq.power_smooth = true;
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_POWER_SMOOTH, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    if (!fq.chunk && fq.n < 512) CHECK(r.chunks == 1, "n %zu: a call shorter than 512 samples is one chunk", fq.n);
    // the pooled power call of the same query: the same route in everything but the kernel
    ForwardQuery pq = fq; pq.power_smooth = false; pq.power_sum = true;
    const ForwardRoute rp = forward_route(pq, [] { return true; });
    CHECK(rp.kernel == FK_POWER_SUM, "the pooled call's kernel");
    CHECK(rp.chunks == r.chunks && rp.len == r.len && rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums &&
          rp.relay_L == r.relay_L && rp.shift == r.shift && rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed &&
          rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map, "n %zu N %zu: not the pooled power call's route", fq.n, fq.nbins);
    // every chunk has a sample and none is longer than len: the table P[0 ... len] covers every index the kernels form
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
  // rows are the power call's
  for (int i = 0; i < 20000; ++i)
  {
    const size_t n = rnd_in(0, 5000), every = rnd_in(1, 600), first = rnd_in(0, 6000);
    size_t rows = 0;
    for (size_t t = first; t < n; t += every) ++rows;
    CHECK(every_rows(n, every, first) == rows, "rows of n %zu every %zu first %zu", n, every, first);
  }
  // the workspace: nothing for one chunk, else one slot per (channel, chunk) of the band's bins, dense and in that order
  CHECK(power_smooth_workspace(3, 1, 100) == 0 && power_smooth_workspace(1, 0, 7) == 0, "a call of one chunk has no workspace");
  for (int i = 0; i < 2000; ++i)
  {
    const size_t ch = rnd_in(1, 5), chunks = rnd_in(2, 40), nb = rnd_in(1, 300);
    CHECK(power_smooth_workspace(ch, chunks, nb) == ch * chunks * nb, "size");
    size_t expect = 0;
    bool dense = true;
    for (size_t c = 0; c < ch; ++c)
      for (size_t j = 0; j < chunks; ++j, expect += nb) dense = dense && power_smooth_slot(c, chunks, j, nb) == expect;
    CHECK(dense && expect == power_smooth_workspace(ch, chunks, nb), "slots tile the workspace");
  }
}

static void test_decay()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double ok : {0.0, 0.5, 0.9, 1.0 - ldexp(1.0, -10), 1.0 - ldexp(1.0, -24), 1e-300, -0.0})
    CHECK(power_smooth_decay_ok<float>(ok) && power_smooth_decay_ok<double>(ok), "decay %.17g is accepted", ok);
  for (double bad : {nan, -nan, inf, -inf, 1.0, 1.5, -1e-30, -0.5})
    CHECK(!power_smooth_decay_ok<float>(bad) && !power_smooth_decay_ok<double>(bad), "decay %.17g is refused", bad);
  // the float case: below 1 as a double, 1 after rounding -- a == 1 never forgets and is refused
  const double near = 1.0 - ldexp(1.0, -26);
  CHECK(near < 1.0 && (float)near == 1.0f, "the case rounds to 1");
  CHECK(!power_smooth_decay_ok<float>(near) && power_smooth_decay_ok<double>(near), "1 - 2^-26: refused for FD float, accepted for FD double");
  CHECK(power_smooth_decay_ok<float>(1.0 - ldexp(1.0, -25)) == ((float)(1.0 - ldexp(1.0, -25)) < 1.0f), "1 - 2^-25 follows its rounding");
  CHECK(!power_smooth_decay_ok<double>(1.0 - ldexp(1.0, -60)), "rounds to 1 on its way into a double literal");
}

template <typename T> static void test_table(const char* name)
{
  const long double u = ldexpl(1.0L, -std::numeric_limits<T>::digits);
  for (double decay : {0.0, 0.5, 0.9, 0.99, 1.0 - ldexp(1.0, -10), 0.123456789, 1e-3})
  {
    const T a = (T)decay;
    for (size_t len : {(size_t)0, (size_t)1, (size_t)2, (size_t)64, (size_t)1160, (size_t)4096})
    {
      const std::vector<T> p = power_smooth_table<T>(a, len);
      CHECK(p.size() == len + 1 && p[0] == (T)1, "%s a %g len %zu: size and P[0]", name, (double)a, len);
      if (len >= 1) CHECK(same_bits(p[1], a), "%s: P[1] is a itself", name);
      long double by_steps = 1.0L;                           // a^j by repeated multiplication in long double
      for (size_t j = 0; j <= len; ++j)
      {
        const long double want = by_steps;
        if (want >= (long double)std::numeric_limits<T>::min())
          CHECK(fabsl((long double)p[j] - want) <= (0.5L + 1e-3L) * u * 2 * want + want * (long double)j * ldexpl(1.0L, -62),
                "%s a %g: P[%zu] = %.20g against %.20Lg", name, (double)a, j, (double)p[j], want);
        else CHECK((long double)p[j] <= (long double)std::numeric_limits<T>::min() && p[j] >= (T)0, "%s: an underflowing power stays small", name);
        if (j) CHECK(p[j] <= p[j - 1], "%s: the table does not grow", name);
        by_steps *= (long double)a;
      }
      if (a == (T)0) for (size_t j = 1; j <= len; ++j) CHECK(same_bits(p[j], (T)0), "%s: decay 0 has P[j >= 1] == +0", name);
    }
  }
}

static void test_fix_rule()
{
  for (int i = 0; i < 3000; ++i)
  {
    const long len = (long)rnd_in(1, 700), shift = (long)rnd_in(0, (size_t)len - 1);
    const size_t n = rnd_in(1, 6000);
    // the walk: chunk after chunk, sample after sample
    size_t t = 0;
    long chunks = (long)((n + (size_t)shift + (size_t)len - 1) / (size_t)len);
    for (long c = 0; c < chunks; ++c)
    {
      const size_t t0 = chunk_begin(c, len, shift), t1 = chunk_end(c, len, shift, n);
      CHECK(t0 == t, "chunks follow one another");
      for (size_t j = 0; t < t1; ++t, ++j)
      {
        const PowerSmoothFix f = power_smooth_fix(t, len, shift);
        if (f.chunk != c || f.power != j + 1) { CHECK(false, "len %ld shift %ld sample %zu: chunk %ld power %zu, the walk says %ld and %zu", len, shift, t, f.chunk, f.power, c, j + 1); break; }
        if (f.power > (size_t)len) CHECK(false, "the power leaves the table");
      }
    }
    CHECK(t == n, "the chunks cover the call");
  }
  // chunk_shift != 0 moves every boundary but the first down
  CHECK(power_smooth_fix(99, 100, 0).chunk == 0 && power_smooth_fix(99, 100, 0).power == 100 && power_smooth_fix(100, 100, 0).chunk == 1 && power_smooth_fix(100, 100, 0).power == 1, "no shift");
  CHECK(power_smooth_fix(92, 100, 7).chunk == 0 && power_smooth_fix(92, 100, 7).power == 93 && power_smooth_fix(93, 100, 7).chunk == 1 && power_smooth_fix(93, 100, 7).power == 1 &&
        power_smooth_fix(193, 100, 7).chunk == 2, "a shift of 7");
}

// the kernels' scheme on the host: chunk 0 from the state, later chunks from +0, the scan of the end values in ascending order, the
// fix-up of the rows of the later chunks -- rows at every sample
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
      std::vector<T> p(n);
      for (size_t t = 0; t < n; ++t) p[t] = (T)((double)(rnd() % 1000003ull) / 1000003.0 * ((t / 500) % 3 == 1 ? 1e4 : 1.0));      // a 40 dB burst
      const T state = trial % 2 ? (T)3.25 : (T)0;
      // the sequential loop in T, and the exact recursion on the same terms and coefficients
      std::vector<T> seq(n);
      std::vector<long double> exact(n);
      volatile T s = state;
      long double x = state, m = state;
      std::vector<long double> big(n);
      for (size_t t = 0; t < n; ++t)
      {
        volatile T as = a * s, bp = b * p[t];
        s = as + bp; seq[t] = s;
        x = (long double)a * x + (long double)b * (long double)p[t]; exact[t] = x;
        m = std::max(m, x); big[t] = m;
      }
      std::vector<T> rows; T end;
      chunked(p, a, state, (long)n, 0, rows, end);
      CHECK(memcmp(rows.data(), seq.data(), n * sizeof(T)) == 0 && same_bits(end, seq[n - 1]), "%s decay %g: one chunk is the sequential loop", name, decay);
      for (long len : {64L, 512L, 333L})
        for (long shift : {0L, 17L})
        {
          chunked(p, a, state, len, shift, rows, end);
          if (a == (T)0) { CHECK(memcmp(rows.data(), seq.data(), n * sizeof(T)) == 0 && same_bits(end, seq[n - 1]), "%s: decay 0 has the loop's bits in any chunking", name); continue; }
          for (size_t t = 0; t < n; ++t)
          {
            const long double bound = 8 * u * big[t] / (1.0L - (long double)a), err = fabsl((long double)rows[t] - exact[t]);
            worst = std::max(worst, err / (u * big[t] / (1.0L - (long double)a)));
            if (err > bound) { CHECK(false, "%s decay %g len %ld shift %ld sample %zu: %Lg beyond %Lg", name, decay, len, shift, t, err, bound); break; }
          }
          CHECK(fabsl((long double)end - exact[n - 1]) <= 8 * u * big[n - 1] / (1.0L - (long double)a), "%s: the end value", name);
        }
    }
  }
  printf("%s: largest chunked error %.3Lf u M / (1 - a)\n", name, worst);
}

int main()
{
  test_route();
  test_sizes();
  test_decay();
  test_table<float>("float");
  test_table<double>("double");
  test_fix_rule();
  test_scheme<float>("float");
  test_scheme<double>("double");
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("power-smooth-logic: all properties hold\n");
  return 0;
}
