// power_peak_logic_test.cpp -- the host-side decisions of the peak-hold analysis (sdft_hip_sdft_power_peak_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the pooled power call's for the same query) and the
// combining rule peak_hold: associative, commutative, NaN-absorbing from either side, with -inf / +inf as the identity of max / min.
// Compiled by tests/test_power_peak_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
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
template <typename T> static bool is_nan(T x) { return x != x; }

// non-negative values as powers are: +0, subnormals, ordinary numbers over many binades, repeats, +inf
template <typename T> static std::vector<T> drawn(size_t count)
{
  std::vector<T> v;
  v.push_back((T)0); v.push_back(std::numeric_limits<T>::denorm_min()); v.push_back(std::numeric_limits<T>::min());
  v.push_back(std::numeric_limits<T>::max()); v.push_back(std::numeric_limits<T>::infinity()); v.push_back((T)1);
  while (v.size() < count)
  {
    const T mant = (T)(rnd() % 1000003ull) / (T)1000003;
    const T x = (T)ldexp((double)mant, (int)rnd_in(0, 60) - 30);
    v.push_back(x);
    if (rnd() % 5 == 0) v.push_back(x);                      // ties
  }
  return v;
}

template <typename T> static void test_rule(const char* name)
{
  const std::vector<T> v = drawn<T>(300);
  const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
  for (int hold = 0; hold < 2; ++hold)
  {
    const T start = hold == kHoldMin ? inf : -inf;
    for (size_t i = 0; i < v.size(); ++i)
    {
      const T a = v[i];
      // the identity: what an empty accumulator holds is replaced by the first term, from either side
      CHECK(same_bits(peak_hold(start, a, hold), a) && same_bits(peak_hold(a, start, hold), a), "%s hold %d: %g against the start value", name, hold, (double)a);
      CHECK(same_bits(peak_hold(a, a, hold), a), "%s hold %d: idempotent", name, hold);
      // NaN absorbs from either side
      CHECK(is_nan(peak_hold(a, nan, hold)), "%s hold %d: a NaN term replaces %g", name, hold, (double)a);
      CHECK(is_nan(peak_hold(nan, a, hold)), "%s hold %d: %g does not replace a held NaN", name, hold, (double)a);
      for (size_t j = 0; j < v.size(); ++j)
      {
        const T b = v[j];
        const T ab = peak_hold(a, b, hold);
        CHECK(same_bits(ab, peak_hold(b, a, hold)), "%s hold %d: commutative on %g, %g", name, hold, (double)a, (double)b);
        CHECK(same_bits(ab, a) || same_bits(ab, b), "%s hold %d: the result is one of the terms", name, hold);
        CHECK(hold == kHoldMin ? (ab <= a && ab <= b) : (ab >= a && ab >= b), "%s hold %d: the extreme of %g, %g", name, hold, (double)a, (double)b);
        CHECK(same_bits(ab, hold == kHoldMin ? (T)fmin((double)a, (double)b) : (T)fmax((double)a, (double)b)), "%s hold %d: fmax / fmin of finite or infinite terms", name, hold);
      }
    }
    // associative: triples drawn from the list (all 300^3 would be 27e6 per type and hold)
    for (int i = 0; i < 200000; ++i)
    {
      const T a = v[rnd_in(0, v.size() - 1)], b = v[rnd_in(0, v.size() - 1)], c = v[rnd_in(0, v.size() - 1)];
      CHECK(same_bits(peak_hold(peak_hold(a, b, hold), c, hold), peak_hold(a, peak_hold(b, c, hold), hold)), "%s hold %d: associative on %g, %g, %g", name, hold,
            (double)a, (double)b, (double)c);
    }
    // ... and with a NaN anywhere in the triple both groupings give NaN
    for (int i = 0; i < 3000; ++i)
    {
      T t[3] = {v[rnd_in(0, v.size() - 1)], v[rnd_in(0, v.size() - 1)], v[rnd_in(0, v.size() - 1)]};
      t[i % 3] = nan;
      const T l = peak_hold(peak_hold(t[0], t[1], hold), t[2], hold), r = peak_hold(t[0], peak_hold(t[1], t[2], hold), hold);
      CHECK(is_nan(l) && is_nan(r), "%s hold %d: a NaN at place %d is lost", name, hold, i % 3);
    }
    // a window in pieces: any cut of a sequence into pieces, pieces combined in any grouping, gives the sequence's extreme
    for (int i = 0; i < 2000; ++i)
    {
      const size_t len = rnd_in(1, 40);
      std::vector<T> w(len);
      for (T& x : w) x = v[rnd_in(0, v.size() - 1)];
      T whole = start;
      for (T x : w) whole = peak_hold(whole, x, hold);
      T joined = start, piece = start;
      bool any = false;
      for (size_t t = 0; t < len; ++t)
      {
        piece = peak_hold(piece, w[t], hold);
        if (t + 1 == len || rnd() % 3 == 0)
        {
          joined = any ? peak_hold(joined, piece, hold) : piece;
          any = true; piece = start;
        }
      }
      CHECK(same_bits(whole, joined), "%s hold %d: a window of %zu samples in pieces", name, hold, len);
    }
  }
  CHECK(peak_hold_ok(0) && peak_hold_ok(1) && !peak_hold_ok(2) && !peak_hold_ok(-1) && !peak_hold_ok(1 << 30), "hold is 0 or 1");
  CHECK(kHoldMax == 0 && kHoldMin == 1, "enum sdft_hip_hold");
}

static void test_route()
{
  CHECK(FK_POWER_PEAK == 11, "get_option(\"last_kernel\") answers 11");
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
    fq.power_peak = true;
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_POWER_PEAK, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    // the pooled power call of the same query: the same route in everything but the kernel
    ForwardQuery pq = fq; pq.power_peak = false; pq.power_sum = true;
    const ForwardRoute rp = forward_route(pq, [] { return true; });
    CHECK(rp.kernel == FK_POWER_SUM, "the pooled call's kernel");
    CHECK(rp.chunks == r.chunks && rp.len == r.len && rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums &&
          rp.relay_L == r.relay_L && rp.shift == r.shift && rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed &&
          rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map, "n %zu N %zu: not the pooled power call's route", fq.n, fq.nbins);
    // ... and the dense power call's chunks, which promise (4) of the header compares against
    ForwardQuery dq = fq; dq.power_peak = false; dq.power = true; dq.power_every = 1;
    const ForwardRoute rd = forward_route(dq, [] { return true; });
    CHECK(rd.chunks == r.chunks && rd.len == r.len && rd.shift == r.shift, "the dense power call's chunks");
  }
}

int main()
{
  test_rule<float>("float");
  test_rule<double>("double");
  test_route();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("power-peak-logic: all properties hold\n");
  return 0;
}
