// power_logic_test.cpp -- the host-side decisions of the power-spectrogram analysis (sdft_hip_sdft_power_n) in sdft_plan_logic.hpp:
// the band's validation, which tiles of the independent-tile geometry form rows, where a power goes, the time chunks of
// forward_power_kernel and the route of the call.  Compiled by tests/test_power_cpu.py with g++ -fsanitize=address,undefined (no HIP).
// Exits non-zero at the first violated property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

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

static void test_band()
{
  const size_t top = (size_t)-1;
  CHECK(power_band_ok(1024, 0, 1024), "all bins");
  CHECK(power_band_ok(1024, 1023, 1), "the last bin");
  CHECK(power_band_ok(1, 0, 1), "a plan of one bin");
  CHECK(!power_band_ok(1024, 0, 0), "an empty band");
  CHECK(!power_band_ok(1024, 1024, 1), "past the last bin");
  CHECK(!power_band_ok(1024, 1, 1024), "one bin too many");
  CHECK(!power_band_ok(1024, 1025, 0), "bin0 past the end");
  CHECK(!power_band_ok(0, 0, 1), "a plan without bins");
  CHECK(!power_band_ok(1024, 1, top), "bin0 + nbins wraps to 0");
  CHECK(!power_band_ok(1024, top, 2), "bin0 + nbins wraps to 1");
  CHECK(!power_band_ok(1024, top / 2 + 1, top / 2 + 1), "bin0 + nbins wraps to 0 from the middle");
  CHECK(!power_band_ok(top, top, 1), "past the largest plan");
  CHECK(power_band_ok(top, top - 1, 1), "the last bin of the largest plan");
  for (int i = 0; i < 20000; ++i)
  {
    const size_t n = rnd_in(0, 300), b = rnd_in(0, 320), k = rnd_in(0, 320);
    CHECK(power_band_ok(n, b, k) == (k >= 1 && b + k <= n), "N %zu band (%zu, %zu)", n, b, k);
  }
}

// every (N, window halo, bins per lane, bin0, nbins) for N <= 300: the predicate against a walk over the lanes of every tile as
// the kernel maps them (lane -> bins kfirst ... kfirst + BPL - 1, halo lanes own nothing), every band bin owned by exactly one
// emitting tile, and the offsets of the band's powers a permutation of [0, rows * nbins)
static void test_tiles()
{
  const int windows[3] = {kWindowBoxcar, kWindowHann, kWindowBlackman};          // halo of 0, 1, 2 bins
  size_t cases = 0;
  for (int wi = 0; wi < 3; ++wi)
    for (int fdx_bytes = 8; fdx_bytes <= 16; fdx_bytes += 8)
    {
      const int window = windows[wi], bpl = bins_per_lane((size_t)fdx_bytes), hl = halo_lanes(window, (size_t)fdx_bytes);
      for (long forced = 0; forced <= 5; forced += 5)                               // the default interior and a small forced one (option "interior")
      {
        const long interior = interior_lanes(window, (size_t)fdx_bytes, forced);
        CHECK(interior >= 1 && interior + 2 * hl <= kLanes, "window %d: %ld interior lanes and %d halo lanes fit a wave", window, interior, hl);
        for (size_t N = 1; N <= 300; ++N)
        {
          const long nt = tiles(N, window, (size_t)fdx_bytes, forced);
          // owner[k]: the tile whose interior lane holds bin k (by the kernel's lane map)
          std::vector<long> owner(N, -1);
          for (long t = 0; t < nt; ++t)
            for (int lane = 0; lane < kLanes; ++lane)
            {
              if (lane < hl || lane >= hl + interior) continue;
              for (int b = 0; b < bpl; ++b)
              {
                const long k = t * interior * bpl + (long)(lane - hl) * bpl + b;
                if (k < 0 || k >= (long)N) continue;
                CHECK(owner[(size_t)k] == -1, "N %zu: bin %ld has two owners", N, k);
                owner[(size_t)k] = t;
              }
            }
          for (size_t k = 0; k < N; ++k) CHECK(owner[k] >= 0, "N %zu: bin %zu has no owner", N, k);
          // bands: all starts with a few lengths for every N, every band for small N
          for (size_t bin0 = 0; bin0 < N; ++bin0)
          {
            const size_t room = N - bin0;
            const size_t lens[6] = {1, 2, 3, room / 2, room > 1 ? room - 1 : 1, room};
            const size_t nl = N <= 40 ? room : 6;
            for (size_t li = 0; li < nl; ++li)
            {
              const size_t nb = N <= 40 ? li + 1 : lens[li];
              if (nb == 0 || nb > room) continue;
              ++cases;
              std::vector<char> brute((size_t)nt, 0);
              for (size_t k = bin0; k < bin0 + nb; ++k) brute[(size_t)owner[k]] = 1;
              for (long t = 0; t < nt; ++t)
                CHECK(power_tile_emits(t, interior, bpl, N, bin0, nb) == (brute[(size_t)t] != 0), "N %zu window %d bpl %d band (%zu, %zu) tile %ld", N, window, bpl, bin0, nb, t);
              // (a bin has one owner, checked above: it is stored exactly once if that tile emits)
              for (size_t k = bin0; k < bin0 + nb; ++k)
                CHECK(power_tile_emits(owner[k], interior, bpl, N, bin0, nb), "N %zu band (%zu, %zu): nobody stores bin %zu", N, bin0, nb, k);
            }
          }
          // a tile past the last one never emits
          CHECK(!power_tile_emits(nt, interior, bpl, N, 0, N), "N %zu: tile %ld does not exist", N, nt);
        }
      }
    }
  CHECK(cases > 500000, "%zu bands walked", cases);
}

static void test_offsets()
{
  for (int i = 0; i < 300; ++i)
  {
    const size_t N = rnd_in(1, 300), bin0 = rnd_in(0, N - 1), nb = rnd_in(1, N - bin0), rows = rnd_in(0, 40), channels = rnd_in(1, 3);
    const size_t stride = power_channel_stride(rows, nb);
    CHECK(stride == rows * nb, "channel stride");
    std::vector<int> hit(channels * rows * nb, 0);
    for (size_t c = 0; c < channels; ++c)
      for (size_t r = 0; r < rows; ++r)
        for (size_t k = bin0; k < bin0 + nb; ++k)
        {
          const size_t o = c * stride + power_offset(r, k, bin0, nb);
          CHECK(o < hit.size(), "offset %zu of %zu", o, hit.size());
          if (o < hit.size()) ++hit[o];
        }
    for (size_t o = 0; o < hit.size(); ++o) CHECK(hit[o] == 1, "N %zu band (%zu, %zu) rows %zu: element %zu written %d times", N, bin0, nb, rows, o, hit[o]);
  }
}

static void test_chunks()
{
  EveryQuery q;
  q.n = 1000000; q.channels = 1; q.tiles = 19; q.compute_units = 256;                 // configs[1]: N = 1024 double, Hann
  for (size_t every : {(size_t)1, (size_t)16, (size_t)100})
  {
    const Chunking c = choose_power_chunks(q, every);
    CHECK(c.len == 1160 && c.chunks == 863, "configs[1], every %zu: %ld chunks of %ld", every, c.chunks, c.len);
  }
  CHECK(power_min_len(1) == kPowerDenseMinLen && power_min_len((size_t)kTimeGroup) == kPowerDenseMinLen, "dense grids");
  CHECK(power_min_len((size_t)kTimeGroup + 1) == kEveryMinLen && power_min_len(100) == kEveryMinLen, "sparse grids");
  q.n = 600;
  Chunking c = choose_power_chunks(q, 1);
  CHECK(c.len == 72 && c.chunks == 9, "a short dense call: %ld chunks of %ld", c.chunks, c.len);
  c = choose_power_chunks(q, 100);
  CHECK(c.len == 304 && c.chunks == 2, "a short sparse call: %ld chunks of %ld", c.chunks, c.len);
  q.n = 511;
  c = choose_power_chunks(q, 1);
  CHECK(c.chunks == 1 && c.len == 511, "calls below kHopSamples are one chunk");
  for (int i = 0; i < 40000; ++i)
  {
    q.n = rnd_in(1, 3000000); q.channels = rnd_in(1, 64); q.tiles = (long)rnd_in(1, 80); q.exact = rnd() & 1;
    q.compute_units = (int)rnd_in(1, 304); q.forced_chunk = (rnd() % 4 == 0) ? (long)rnd_in(1, 5000) : 0;
    const size_t every = (rnd() & 1) ? rnd_in(1, 8) : rnd_in(9, 5000);
    c = choose_power_chunks(q, every);
    CHECK(c.len >= 1 && c.chunks >= 1 && (size_t)c.chunks <= q.n, "n %zu: %ld chunks", q.n, c.chunks);
    CHECK((size_t)(c.chunks - 1) * (size_t)c.len < q.n && (size_t)c.chunks * (size_t)c.len >= q.n, "n %zu: %ld chunks of %ld cover the call once", q.n, c.chunks, c.len);
    if (q.forced_chunk == 0)
    {
      const long least = std::min<long>(power_min_len(every), (long)q.n);
      CHECK(c.len >= least || c.chunks == 1, "n %zu every %zu: chunks of %ld, shorter than %ld", q.n, every, c.len, least);
      if (q.n < (size_t)kHopSamples) CHECK(c.chunks == 1, "n %zu: one chunk", q.n);
      if (q.exact && c.chunks > 1) CHECK(c.len % 128 == 0, "exact: whole relay blocks (%ld)", c.len);
    }
  }
}

// the route of the call: forward_power_kernel whatever the shape, never the hop, row-group, self-carried, flow or pipelined forms
static void test_route()
{
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery q;
    q.n = rnd_in(1, 2000000); q.nbins = rnd_in(1, 4200); q.channels = rnd_in(1, 8);
    const bool f32 = rnd() & 1;
    q.fd_bytes = f32 ? 4 : 8; q.fdx_bytes = f32 ? 8 : 16;
    q.window = (int)rnd_in(0, 3); q.cursor = rnd_in(0, 2 * q.nbins - 1); q.exact = f32 || (rnd() & 1); q.fid_canonical = rnd() & 1;
    q.power = true; q.power_every = rnd_in(1, 3000);
    q.analysis_batch = rnd() & 1; q.pipe_wanted = rnd() & 1;
    bool asked = false;
    const ForwardRoute r = forward_route(q, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_POWER, "n %zu N %zu: kernel %d", q.n, q.nbins, r.kernel);
    CHECK(!r.self && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", q.n, q.nbins);
    CHECK(r.chunks >= 1 && r.segments >= 1 && r.segments <= r.chunks, "n %zu: %ld segments of %ld chunks", q.n, r.segments, r.chunks);
    CHECK(r.tiles == tiles(q.nbins, q.window, q.fdx_bytes, 0), "tiles");
    // the same query as a decimated analysis differs in the kernel only when the grid is sparse
    ForwardQuery e = q; e.power = false; e.every = true;
    const ForwardRoute re = forward_route(e, [] { return true; });
    CHECK(re.kernel == FK_EVERY, "the decimated analysis keeps its kernel");
    if (q.power_every > (size_t)kTimeGroup) CHECK(re.chunks == r.chunks && re.len == r.len && re.carry == r.carry && re.relay_L == r.relay_L, "sparse grids: the decimated analysis' chunks");
  }
  CHECK(FK_POWER == 5, "get_option(\"last_kernel\") answers 5");
}

int main()
{
  test_band();
  test_tiles();
  test_offsets();
  test_chunks();
  test_route();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("power-logic: all properties hold\n");
  return 0;
}
