// band_peak_logic_test.cpp -- the host-side decisions of the band-peak analysis (sdft_hip_sdft_band_peak_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the filterbank call's for the same query: the tile form and
// choose_power_chunks), the rows of a launch (filterbank_segment_rows with a slot of two numbers), the refusal of plans whose bins
// are no exact numbers of FD, and the rule itself: logic::band_peak_take over vectors the test draws in numpy.
// Compiled by tests/test_band_peak_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.
//
// usage: band_peak_logic_test                                  the properties
//        band_peak_logic_test <f32|f64> <len> <in.raw> <out.raw>    the rule: in.raw holds vectors of <len> numbers; out.raw receives
//                                                               per vector three int64: the bin of one walk, of a walk cut into
//                                                               pieces at every multiple of 7, and of one cut at drawn places

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

// the filterbank call of the same query: the same route in everything but the kernel
static void same_route_as_filterbank(const ForwardQuery& fq)
{
  bool asked = false;
  const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
  CHECK(r.kernel == FK_BAND_PEAK, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
  // the tile form only: never resident, pipelined or fused; no self-carried chunks, no prefix cells, no flow mode
  CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
  ForwardQuery pq = fq; pq.band_peak = false; pq.filterbank = true;
  const ForwardRoute rp = forward_route(pq, [] { return true; });
  CHECK(rp.kernel == FK_FILTERBANK, "the filterbank call's kernel");
  CHECK(rp.chunks == r.chunks && rp.len == r.len, "n %zu N %zu ch %zu: chunks %ld x %ld, the filterbank call's %ld x %ld", fq.n, fq.nbins, fq.channels, r.chunks, r.len, rp.chunks, rp.len);
  CHECK(rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums && rp.relay_L == r.relay_L && rp.shift == r.shift &&
        rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed && rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map,
        "n %zu N %zu: not the filterbank call's route", fq.n, fq.nbins);
  // the chunk choice is choose_power_chunks of the query the route builds, nothing else
  EveryQuery e;
  e.n = fq.n; e.channels = std::max<size_t>(fq.channels, 1); e.tiles = tiles(fq.nbins, fq.window, fq.fdx_bytes, fq.interior); e.exact = fq.exact;
  e.forced_chunk = fq.chunk; e.compute_units = fq.compute_units;
  const Chunking c = choose_power_chunks(e, fq.power_every);
  // (the relay form of the exact carries shifts the chunks' starts, which may add one chunk: the filterbank call's route likewise)
  CHECK(c.len == r.len && (c.chunks == r.chunks || (r.shift && c.chunks + 1 == r.chunks)), "n %zu N %zu: %ld x %ld shifted by %u, choose_power_chunks says %ld x %ld",
        fq.n, fq.nbins, r.chunks, r.len, r.shift, c.chunks, c.len);
}

static void test_route()
{
  CHECK(FK_BAND_PEAK == 14, "get_option(\"last_kernel\") answers 14");
  CHECK(FK_POWER_MOMENTS == 13 && FK_LAG_SUM == 12 && FK_POWER_PEAK == 11 && FK_MIX == 10 && FK_CROSS_SUM == 8 && FK_FILTERBANK == 7 && FK_POWER_SUM == 6,
        "the other kernels keep their numbers");
  for (size_t n : {(size_t)1000000, (size_t)600, (size_t)511})
    for (size_t every : {(size_t)1, (size_t)100})
    {
      ForwardQuery fq;
      fq.n = n; fq.nbins = 1024; fq.channels = 1; fq.fd_bytes = 8; fq.fdx_bytes = 16; fq.window = 1; fq.compute_units = 256; fq.band_peak = true; fq.power_every = every;
      same_route_as_filterbank(fq);
      const ForwardRoute r = forward_route(fq, [] { return true; });
      if (n == 511) CHECK(r.chunks == 1 && r.len == 511, "calls below kHopSamples are one chunk");
    }
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery fq;
    fq.n = rnd_in(1, 2000000); fq.nbins = rnd_in(1, 4200); fq.channels = rnd_in(1, 8);
    const bool f32 = rnd() & 1;
    fq.fd_bytes = f32 ? 4 : 8; fq.fdx_bytes = f32 ? 8 : 16;
    fq.window = (int)rnd_in(0, 3); fq.cursor = rnd_in(0, 2 * fq.nbins - 1); fq.exact = f32 || (rnd() & 1); fq.fid_canonical = rnd() & 1;
    fq.analysis_batch = rnd() & 1; fq.pipe_wanted = rnd() & 1;
    fq.compute_units = (int)rnd_in(1, 304);
    if (rnd() % 4 == 0) fq.chunk = (long)rnd_in(1, 5000);
    if (rnd() % 4 == 0) fq.segments = (long)rnd_in(0, 4);
    if (rnd() % 4 == 0) fq.chain = (long)rnd_in(0, 2);
    fq.band_peak = true;
    fq.power_every = rnd() & 1 ? 1 : rnd_in(1, fq.n);
    same_route_as_filterbank(fq);
  }
}

static void test_workspace()
{
  CHECK(kBandPeakPair == 2, "a slot holds the value and the bin");
  for (int i = 0; i < 20000; ++i)
  {
    const size_t ch = rnd_in(0, 9), nslots = rnd_in(0, 5000), fd = rnd() & 1 ? 4 : 8;
    const size_t bound = rnd() & 1 ? kFilterbankWorkspaceBytes : rnd_in(1, (size_t)1 << 28);
    const size_t rows = band_peak_segment_rows(ch, nslots, fd, bound);
    CHECK(rows == filterbank_segment_rows(ch, nslots, 2 * fd, bound), "filterbank_segment_rows with a slot of 2 * sizeof(FD)");
    CHECK(rows >= 1, "a launch keeps one row at least");
    if (nslots == 0) { CHECK(rows == (size_t)-1, "no split band: no bound"); continue; }
    const size_t c1 = std::max<size_t>(ch, 1), row_bytes = c1 * nslots * 2 * fd;
    CHECK(rows == 1 || rows * row_bytes <= bound, "the rows of a launch stay within the bound");
    CHECK((rows + 1) * row_bytes > bound, "and are as many as fit");
    CHECK(rows <= filterbank_segment_rows(ch, nslots, fd, bound), "never more rows than the filterbank call's launch");
    const size_t r = rnd_in(1, 3000);
    CHECK(band_peak_workspace(c1, r, nslots) == 2 * filterbank_workspace(c1, r, nslots), "[channels][rows][nslots] pairs");
    // the last pair of the last slot ends inside the workspace
    CHECK(2 * filterbank_slot(c1 - 1, r, r - 1, nslots, nslots - 1) + 2 == band_peak_workspace(c1, r, nslots), "the last slot's pair is the workspace's last");
  }
  CHECK(band_peak_segment_rows(1, 1024, 8) == kFilterbankWorkspaceBytes / (1024 * 16), "64 MiB of double pairs");
}

static void test_exact_bins()
{
  CHECK(band_peak_bins_exact((size_t)1 << 24, 4) && !band_peak_bins_exact(((size_t)1 << 24) + 1, 4), "FD float: dftsize <= 2^24");
  CHECK(band_peak_bins_exact(((size_t)1 << 24) + 1, 8) && band_peak_bins_exact((size_t)1 << 40, 8), "FD double holds every bin a plan can have");
  CHECK((float)(((size_t)1 << 24) - 1) == 16777215.0f && (size_t)(float)(((size_t)1 << 24) - 1) == ((size_t)1 << 24) - 1, "the last bin of the largest FD float plan is exact");
}

// the rule over [a, b): the held pair starts at a
template <typename T> static void walk(const T* v, size_t a, size_t b, T& m, size_t& at)
{
  m = v[a]; at = a;
  for (size_t k = a + 1; k < b; ++k)
    if (band_peak_take(m, v[k])) { m = v[k]; at = k; }
}
// pieces joined in ascending order: the lower piece is held, the higher one the candidate
template <typename T> static size_t joined(const T* v, size_t len, const std::vector<size_t>& cuts)
{
  T m = 0; size_t at = 0;
  for (size_t i = 0; i + 1 < cuts.size(); ++i)
  {
    T pm; size_t pat;
    walk(v, cuts[i], cuts[i + 1], pm, pat);
    if (i == 0 || band_peak_take(m, pm)) { m = pm; at = pat; }
  }
  (void)len;
  return at;
}
template <typename T> static int rule(size_t len, const char* in, const char* out)
{
  FILE* f = fopen(in, "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const size_t count = (size_t)ftell(f) / (len * sizeof(T));
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(count * len);
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) return 3;
  fclose(f);
  std::vector<long long> bins(count * 3);
  for (size_t i = 0; i < count; ++i)
  {
    const T* row = v.data() + i * len;
    T m; size_t at;
    walk(row, 0, len, m, at);
    bins[3 * i] = (long long)at;
    if (memcmp(&m, row + at, sizeof(T)) != 0 && m == m) return 4;      // the value is the bin's, bit for bit
    std::vector<size_t> sevens, drawn;
    for (size_t k = 0; k < len; k += 7) sevens.push_back(k);
    sevens.push_back(len);
    drawn.push_back(0);
    for (size_t k = 1; k < len; ++k) if (rnd() % 3 == 0) drawn.push_back(k);
    drawn.push_back(len);
    bins[3 * i + 1] = (long long)joined(row, len, sevens);
    bins[3 * i + 2] = (long long)joined(row, len, drawn);
  }
  f = fopen(out, "wb");
  if (!f) return 3;
  fwrite(bins.data(), sizeof(long long), bins.size(), f);
  fclose(f);
  printf("band-peak-rule: %zu vectors of %zu\n", count, len);
  return 0;
}

int main(int argc, char* argv[])
{
  if (argc == 5)
  {
    const size_t len = (size_t)atol(argv[2]);
    if (len == 0) return 2;
    return strcmp(argv[1], "f32") == 0 ? rule<float>(len, argv[3], argv[4]) : rule<double>(len, argv[3], argv[4]);
  }
  test_route();
  test_workspace();
  test_exact_bins();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("band-peak-logic: all properties hold\n");
  return 0;
}
