// power_moments_logic_test.cpp -- the host-side decisions of the power-moments analysis (sdft_hip_sdft_power_moments_n) in
// sdft_plan_logic.hpp: the kernel id, the route and the time chunks (the pooled power call's for the same query: the call has no
// chunk choice of its own), the workspace of cut windows (the cross-spectrum call's with channels for pairs) and the bounds of the
// host segments (rows of twice the pooled call's bytes).
// Compiled by tests/test_power_moments_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.

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

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static size_t rnd_in(size_t lo, size_t hi) { return lo + (size_t)(rnd() % (unsigned long long)(hi - lo + 1)); }

// the pooled power call of the same query: the same route in everything but the kernel, the chunk choice first of all
static void same_route_as_pooled(const ForwardQuery& fq)
{
  bool asked = false;
  const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
  CHECK(r.kernel == FK_POWER_MOMENTS, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
  // never resident, pipelined or fused; no self-carried chunks, no prefix cells, no flow mode
  CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
  ForwardQuery pq = fq; pq.power_moments = false; pq.cross_items = 0; pq.power_sum = true;
  const ForwardRoute rp = forward_route(pq, [] { return true; });
  CHECK(rp.kernel == FK_POWER_SUM, "the pooled call's kernel");
  CHECK(rp.chunks == r.chunks && rp.len == r.len, "n %zu N %zu ch %zu: chunks %ld x %ld, the pooled call's %ld x %ld", fq.n, fq.nbins, fq.channels, r.chunks, r.len, rp.chunks, rp.len);
  CHECK(rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums && rp.relay_L == r.relay_L && rp.shift == r.shift &&
        rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed && rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map,
        "n %zu N %zu: not the pooled power call's route", fq.n, fq.nbins);
  // the chunk choice is choose_power_sum_chunks of the query the route builds, nothing else
  EveryQuery e;
  e.n = fq.n; e.channels = std::max<size_t>(fq.channels, 1); e.tiles = tiles(fq.nbins, fq.window, fq.fdx_bytes, fq.interior); e.exact = fq.exact;
  e.forced_chunk = fq.chunk; e.compute_units = fq.compute_units;
  const Chunking c = choose_power_sum_chunks(e);
  // (the relay form of the exact carries shifts the chunks' starts, which may add one chunk: the pooled call's route likewise)
  CHECK(c.len == r.len && (c.chunks == r.chunks || (r.shift && c.chunks + 1 == r.chunks)), "n %zu N %zu: %ld x %ld shifted by %u, choose_power_sum_chunks says %ld x %ld",
        fq.n, fq.nbins, r.chunks, r.len, r.shift, c.chunks, c.len);
  // the item count of another call's table does not reach the route
  ForwardQuery oq = fq; oq.cross_items = 1000;
  const ForwardRoute ro = forward_route(oq, [] { return true; });
  CHECK(ro.chunks == r.chunks && ro.len == r.len && ro.segments == r.segments, "cross_items moved the route");
}

static void test_route()
{
  CHECK(FK_POWER_MOMENTS == 13, "get_option(\"last_kernel\") answers 13");
  CHECK(FK_LAG_SUM == 12 && FK_POWER_PEAK == 11 && FK_MIX == 10 && FK_CROSS_SUM == 8 && FK_POWER_SUM == 6, "the other kernels keep their numbers");
  // the fixed queries of tests/cpp/power_sum_logic_test.cpp: configs[1] (N = 1024 double, Hann: 19 tiles), a short call, a call
  // below kHopSamples
  for (size_t n : {(size_t)1000000, (size_t)600, (size_t)511})
  {
    ForwardQuery fq;
    fq.n = n; fq.nbins = 1024; fq.channels = 1; fq.fd_bytes = 8; fq.fdx_bytes = 16; fq.window = 1; fq.compute_units = 256; fq.power_moments = true;
    CHECK(tiles(fq.nbins, fq.window, fq.fdx_bytes, fq.interior) == 19, "configs[1] has 19 tiles");
    same_route_as_pooled(fq);
    const ForwardRoute r = forward_route(fq, [] { return true; });
    if (n == 1000000) CHECK(r.len == 1160 && r.chunks == 863, "configs[1]: %ld chunks of %ld", r.chunks, r.len);
    if (n == 600) CHECK(r.len == 72 && r.chunks == 9, "a short call is cut at the dense minimum: %ld chunks of %ld", r.chunks, r.len);
    if (n == 511) CHECK(r.chunks == 1 && r.len == 511, "calls below kHopSamples are one chunk");
  }
  // ... and its drawn ones
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
    fq.power_moments = true;
    fq.cross_items = fq.channels;                            // (what the plan passes: its channels take the pairs' place)
    same_route_as_pooled(fq);
  }
}

static void test_workspace()
{
  for (int i = 0; i < 5000; ++i)
  {
    const size_t ch = rnd_in(1, 9), chunks = rnd_in(1, 900), nb = rnd_in(1, 4096);
    CHECK(power_moments_workspace(ch, chunks, nb) == cross_sum_workspace(ch, chunks, nb), "the cross-spectrum call's workspace with channels for pairs");
    CHECK(power_moments_workspace(ch, chunks, nb) == power_sum_workspace(ch, chunks, 2 * nb), "[channels][chunks][2][nbins] pairs");
    CHECK(power_moments_workspace(0, chunks, nb) == power_moments_workspace(1, chunks, nb), "a single-channel plan is one channel");
    const size_t c = rnd_in(0, ch - 1), k = rnd_in(0, chunks - 1);
    for (int slot = 0; slot < 2; ++slot)
    {
      const size_t at = power_moments_slot(c, chunks, k, slot, nb);
      CHECK(at == cross_sum_slot(c, chunks, k, slot, nb), "the cross-spectrum call's slot");
      CHECK(at == ((c * chunks + k) * 2 + (size_t)slot) * 2 * nb, "slot (%zu, %zu, %d)", c, k, slot);
      if (chunks > 1) CHECK(at + 2 * nb <= power_moments_workspace(ch, chunks, nb), "slot (%zu, %zu, %d) ends inside the workspace", c, k, slot);
      else CHECK(power_moments_workspace(ch, chunks, nb) == 0, "a call of one chunk cuts no window");
    }
    const size_t rows = rnd_in(0, 5000);
    CHECK(power_moments_channel_stride(rows, nb) == rows * 2 * nb && power_moments_channel_stride(rows, nb) == cross_pair_stride(rows, nb),
          "a channel's moments are dense [rows][nbins][2]");
  }
}

static void test_segments()
{
  for (int i = 0; i < 20000; ++i)
  {
    const size_t n = rnd_in(1, 300000), ch = rnd_in(1, 6), nb = rnd_in(1, 2048);
    const size_t every = rnd_in(1, n), first = rnd() % 3 == 0 ? 0 : rnd_in(0, n + 10);
    const size_t fd = rnd() & 1 ? 4 : 8, td = rnd() & 1 ? 4 : 8;
    const size_t stage = rnd_in(1, 1 << 22);
    const bool xd = rnd() & 1, od = rnd() & 1;
    const size_t seg = power_moments_segment(n, every, first, ch, nb, fd, td, stage, xd, od);
    CHECK(seg >= 1, "n %zu: a segment is never empty", n);
    CHECK(seg <= n, "seg %zu of n %zu", seg, n);
    size_t covered = 0, segments = 0;
    for (size_t t = 0; t < n; t += seg) { covered += std::min(seg, n - t); ++segments; }
    CHECK(covered == n && segments == (n + seg - 1) / seg, "the segments cover the call once");
    if (xd && od) CHECK(seg == n, "device pointers are one segment");
    // the pooled call's rule on rows of twice its bytes: channels * nbins pairs
    const size_t row_bytes = ch * 2 * nb * fd;
    CHECK(seg == grid_segment(n, every, first, row_bytes, ch * td, stage, xd, od, true), "grid_segment on the doubled row");
    CHECK(seg == lag_sum_segment(n, every, first, ch, nb, fd, td, stage, xd, od), "the lag-product call's segments: the same row bytes");
    CHECK(seg <= grid_segment(n, every, first, row_bytes / 2, ch * td, stage, xd, od, true), "never longer than the pooled call's segment of the same grid");
    // what a segment writes and reads stays within stage_bytes wherever one row does
    if (!od && row_bytes <= stage) CHECK((seg / every) * row_bytes <= stage || seg < every, "rows of a segment within stage_bytes");
    if (!xd && seg > (size_t)kHopSamples) CHECK(seg * ch * td <= stage, "samples of a segment within stage_bytes");
    if (seg < n && seg > every && first % every == 0) CHECK(seg % every == 0, "whole windows where the grid allows it");
  }
}

int main()
{
  test_route();
  test_workspace();
  test_segments();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("power-moments-logic: all properties hold\n");
  return 0;
}
