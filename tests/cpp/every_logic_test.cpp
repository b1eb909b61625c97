// every_logic_test.cpp -- the host-side decisions of the decimated analysis (sdft_hip_sdft_every_n) in sdft_plan_logic.hpp: the
// row count, the first of the next call and of a segment, the time chunks of forward_every_kernel.  Compiled by
// tests/test_every_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

using namespace sdfthip::logic;

static int failures = 0;
#define CHECK(cond, ...)                                                                    \
  do {                                                                                      \
    if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
      if (failures > 20) exit(1); }                                                         \
  } while (0)

static unsigned long long rng_state = 0x2545F4914F6CDD1Dull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static size_t rnd_in(size_t lo, size_t hi) { return lo + (size_t)(rnd() % (unsigned long long)(hi - lo + 1)); }

// the grid by enumeration
static size_t count_rows(size_t n, size_t every, size_t first)
{
  size_t r = 0;
  for (size_t t = first; t < n; t += every) ++r;
  return r;
}

static void test_rows()
{
  CHECK(every_rows(0, 1, 0) == 0, "no samples, no rows");
  CHECK(every_rows(10, 0, 0) == 0, "every == 0 keeps nothing");
  CHECK(every_rows(10, 1, 0) == 10, "every row");
  CHECK(every_rows(10, 3, 0) == 4, "0 3 6 9");
  CHECK(every_rows(10, 3, 2) == 3, "2 5 8");
  CHECK(every_rows(10, 3, 9) == 1, "9");
  CHECK(every_rows(10, 3, 10) == 0, "first == n");
  CHECK(every_rows(10, 100, 0) == 1, "every > n");
  CHECK(every_rows(1000000, 100, 0) == 10000, "the full-size shape");
  CHECK(every_rows(48000, 4000, 3999) == 12, "examples/spectrogram.cpp");
  CHECK(every_rows((size_t)-1, (size_t)-1, 0) == 1, "no overflow at the top of the range");
  for (int i = 0; i < 20000; ++i)
  {
    const size_t n = rnd_in(0, 3000), every = rnd_in(1, 400), first = rnd_in(0, 3500);
    CHECK(every_rows(n, every, first) == count_rows(n, every, first), "n %zu every %zu first %zu", n, every, first);
  }
}

// calls of any length with first carried as documented give the grid of one long call
static void test_streaming()
{
  for (int trial = 0; trial < 2000; ++trial)
  {
    const size_t every = rnd_in(1, 300), first0 = rnd_in(0, 600);
    size_t t = 0, first = first0, rows = 0;
    const int calls = (int)rnd_in(1, 12);
    for (int c = 0; c < calls; ++c)
    {
      const size_t n = rnd_in(0, 900);
      // the rows of this call sit at global samples t + first + k * every, which must be the long call's grid
      const size_t r = every_rows(n, every, first);
      for (size_t k = 0; k < r; ++k)
      {
        const size_t g = t + first + k * every;
        CHECK(g >= first0 && (g - first0) % every == 0 && (g - first0) / every == rows + k, "row %zu of call %d at %zu", k, c, g);
      }
      rows += r;
      first = every_next_first(n, every, first);
      t += n;
    }
    CHECK(rows == every_rows(t, every, first0), "every %zu first %zu: %zu rows in calls, %zu in one", every, first0, rows, every_rows(t, every, first0));
  }
  CHECK(every_next_first(100, 7, 0) == 5, "0 .. 98, next 105");
  CHECK(every_next_first(100, 7, 150) == 50, "no row: first - n");
  CHECK(every_next_first(100, 100, 0) == 0, "hop-aligned");
}

static void test_segments()
{
  for (int i = 0; i < 20000; ++i)
  {
    const size_t every = rnd_in(1, 300), first = rnd_in(0, 2000), t0 = rnd_in(0, 3000);
    const size_t f = every_first_from(t0, every, first);
    const size_t g = t0 + f;                                    // the grid's first sample at or after t0
    CHECK(g >= first && (g - first) % every == 0, "t0 %zu every %zu first %zu: %zu on the grid", t0, every, first, g);
    CHECK(g < every + std::max(first, t0), "t0 %zu every %zu first %zu: %zu is the first", t0, every, first, g);
    if (g >= every) CHECK(g - every < t0 || g - every < first, "t0 %zu every %zu first %zu: nothing earlier", t0, every, first);
  }
}

static void test_chunks()
{
  EveryQuery q;
  q.n = 1000000; q.channels = 1; q.tiles = 19; q.compute_units = 256;                 // configs[1]: N = 1024 double, Hann
  Chunking c = choose_every_chunks(q);
  CHECK(c.chunks * q.tiles >= 16384 && c.chunks * q.tiles < 16384 + 2 * q.tiles, "configs[1]: %ld chunks x %ld tiles fill 256 CUs", c.chunks, q.tiles);
  CHECK(c.len == 1160 && c.chunks == 863, "configs[1]: %ld chunks of %ld", c.chunks, c.len);
  q.n = 262144; q.tiles = 37; q.exact = true;                                          // configs[2]: N = 4096 float, Blackman
  c = choose_every_chunks(q);
  CHECK(c.len == 640 && c.chunks == 410, "configs[2]: %ld chunks of %ld, whole relay blocks", c.chunks, c.len);
  q.n = 511; q.exact = false;
  c = choose_every_chunks(q);
  CHECK(c.chunks == 1 && c.len == 511, "short calls are one chunk");
  q.n = 600;
  c = choose_every_chunks(q);
  CHECK(c.chunks == 2 && c.len == 304, "chunks of at least kEveryMinLen: %ld of %ld", c.chunks, c.len);
  q.forced_chunk = 100;
  c = choose_every_chunks(q);
  CHECK(c.len == 104 && c.chunks == 6, "option chunk (direct sums: whole blocks of 8): %ld of %ld", c.chunks, c.len);
  q.forced_chunk = 0; q.n = 0;
  c = choose_every_chunks(q);
  CHECK(c.chunks == 1, "empty call");
  for (int i = 0; i < 20000; ++i)
  {
    q.n = rnd_in(1, 3000000); q.channels = rnd_in(1, 64); q.tiles = (long)rnd_in(1, 80); q.exact = rnd() & 1;
    q.compute_units = (int)rnd_in(1, 304); q.forced_chunk = (rnd() % 4 == 0) ? (long)rnd_in(1, 5000) : 0;
    c = choose_every_chunks(q);
    CHECK(c.len >= 1 && c.chunks >= 1 && (size_t)(c.chunks - 1) * (size_t)c.len < q.n && (size_t)c.chunks * (size_t)c.len >= q.n,
          "n %zu: %ld chunks of %ld cover the call once", q.n, c.chunks, c.len);
    if (q.forced_chunk == 0 && q.n >= (size_t)kHopSamples)
    {
      CHECK(c.len >= std::min<long>(kEveryMinLen, (long)q.n) || c.chunks == 1, "n %zu: chunks of %ld", q.n, c.len);
      const long waves = c.chunks * (long)q.channels * q.tiles, target = (long)q.compute_units * kEverySimds * kEveryWavesPerSimd;
      CHECK(2 * waves >= target || c.len <= 4 * kEveryMinLen, "n %zu: %ld waves for %ld", q.n, waves, target);
      if (q.exact && c.chunks > 1) CHECK(c.len % 128 == 0, "exact: whole relay blocks (%ld)", c.len);
    }
  }
}

int main()
{
  test_rows();
  test_streaming();
  test_segments();
  test_chunks();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("every-logic: all properties hold\n");
  return 0;
}
