// lag_sum_logic_test.cpp -- the host-side decisions of the lag-product analysis (sdft_hip_sdft_lag_sum_n) in sdft_plan_logic.hpp:
// the kernel id, the route flags and the time chunks (the pooled power call's for the same query), the workspace of cut windows
// (the cross-spectrum call's with channels for pairs), the bounds of the host segments, and the row counts and the next call's
// first (power_sum_rows / every_next_first along a stream cut into calls).
// Compiled by tests/test_lag_sum_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.

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

static void test_route()
{
  CHECK(FK_LAG_SUM == 12, "get_option(\"last_kernel\") answers 12");
  CHECK(FK_POWER_PEAK == 11 && FK_MIX == 10 && FK_CROSS_SUM == 8 && FK_POWER_SUM == 6, "the other kernels keep their numbers");
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
    fq.lag_sum = true;
    fq.cross_items = fq.channels;                            // (what the plan passes: its channels take the pairs' place)
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_LAG_SUM, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    // never resident, pipelined or fused; no self-carried chunks, no prefix cells, no flow mode
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    // the pooled power call of the same query: the same route in everything but the kernel, the chunk choice first of all
    ForwardQuery pq = fq; pq.lag_sum = false; pq.cross_items = 0; pq.power_sum = true;
    const ForwardRoute rp = forward_route(pq, [] { return true; });
    CHECK(rp.kernel == FK_POWER_SUM, "the pooled call's kernel");
    CHECK(rp.chunks == r.chunks && rp.len == r.len, "n %zu N %zu ch %zu: chunks %ld x %ld, the pooled call's %ld x %ld", fq.n, fq.nbins, fq.channels, r.chunks, r.len, rp.chunks, rp.len);
    CHECK(rp.tiles == r.tiles && rp.interior == r.interior && rp.carry == r.carry && rp.sums == r.sums && rp.relay_L == r.relay_L && rp.shift == r.shift &&
          rp.segments == r.segments && rp.delta_in_carry == r.delta_in_carry && rp.use_seed == r.use_seed && rp.vec_store == r.vec_store && rp.xcd_map == r.xcd_map,
          "n %zu N %zu: not the pooled power call's route", fq.n, fq.nbins);
    // the item count of another call's table does not reach the lag route
    ForwardQuery oq = fq; oq.cross_items = 1000;
    const ForwardRoute ro = forward_route(oq, [] { return true; });
    CHECK(ro.chunks == r.chunks && ro.len == r.len && ro.segments == r.segments, "cross_items moved the lag route");
  }
  // a call of one chunk below 512 samples: bit-identical, whatever else
  ForwardQuery s; s.n = 300; s.nbins = 64; s.channels = 1; s.fd_bytes = 8; s.fdx_bytes = 16; s.window = 1; s.lag_sum = true;
  const ForwardRoute rs = forward_route(s, [] { return true; });
  CHECK(rs.kernel == FK_LAG_SUM && rs.chunks == 1 && rs.len == 300, "a short call is one chunk");
}

static void test_workspace()
{
  for (int i = 0; i < 5000; ++i)
  {
    const size_t ch = rnd_in(1, 9), chunks = rnd_in(1, 900), nb = rnd_in(1, 4096);
    CHECK(lag_sum_workspace(ch, chunks, nb) == cross_sum_workspace(ch, chunks, nb), "the cross-spectrum call's workspace with channels for pairs");
    CHECK(lag_sum_workspace(ch, chunks, nb) == power_sum_workspace(ch, chunks, 2 * nb), "[channels][chunks][2][nbins] complex");
    CHECK(lag_sum_workspace(0, chunks, nb) == lag_sum_workspace(1, chunks, nb), "a single-channel plan is one channel");
    const size_t c = rnd_in(0, ch - 1), k = rnd_in(0, chunks - 1);
    for (int slot = 0; slot < 2; ++slot)
    {
      const size_t at = lag_sum_slot(c, chunks, k, slot, nb);
      CHECK(at == ((c * chunks + k) * 2 + (size_t)slot) * 2 * nb, "slot (%zu, %zu, %d)", c, k, slot);
      if (chunks > 1) CHECK(at + 2 * nb <= lag_sum_workspace(ch, chunks, nb), "slot (%zu, %zu, %d) ends inside the workspace", c, k, slot);
      else CHECK(lag_sum_workspace(ch, chunks, nb) == 0, "a call of one chunk cuts no window");
    }
    const size_t rows = rnd_in(0, 5000);
    CHECK(lag_channel_stride(rows, nb) == rows * 2 * nb, "a channel's sums are dense [rows][nbins] complex");
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
    const size_t seg = lag_sum_segment(n, every, first, ch, nb, fd, td, stage, xd, od);
    CHECK(seg >= 1 && seg <= n, "seg %zu of n %zu", seg, n);
    if (xd && od) CHECK(seg == n, "device pointers are one segment");
    // the cross-spectrum call's bounds with npairs = channels (sdft_cross_sum_n)
    const size_t row_bytes = ch * 2 * nb * fd;
    size_t want = n;
    if (!od) want = std::min(want, stage_rows(n, row_bytes, stage) * every);
    if (!xd) want = std::min(want, std::max<size_t>((size_t)kHopSamples, stage_rows(n, ch * td, stage)));
    if (want < n && want > every && first % every == 0) want -= want % every;
    CHECK(seg == want, "n %zu every %zu first %zu: seg %zu, the cross-spectrum call's %zu", n, every, first, seg, want);
    // what a segment writes stays within stage_bytes wherever one row does: (seg + every - 1) / every + 1 rows at the most, of
    // which the head goes to a buffer of its own
    if (!od && row_bytes <= stage) CHECK((seg / every) * row_bytes <= stage || seg < every, "rows of a segment within stage_bytes");
    if (!xd && seg > (size_t)kHopSamples) CHECK(seg * ch * td <= stage, "samples of a segment within stage_bytes");
    if (seg < n && seg > every && first % every == 0) CHECK(seg % every == 0, "whole windows where the grid allows it");
  }
}

// rows and the next first along a stream cut into calls: the rows of the calls, with every head row (first > 0 after the first
// call) counted into the row before it, are the rows of one long call; the next first is every_next_first's
static void test_rows_and_next_first()
{
  for (int i = 0; i < 20000; ++i)
  {
    const size_t n = rnd_in(1, 5000), every = rnd_in(1, 1200), first0 = rnd() % 3 == 0 ? 0 : rnd_in(0, 1500);
    const size_t whole = power_sum_rows(n, every, first0);
    CHECK(whole == (first0 > 0 ? 1u : 0u) + every_rows(n, every, first0), "rows = head + rows of sdft_hip_sdft_every_n");
    CHECK(power_sum_rows(0, every, first0) == 0, "no samples, no rows");
    size_t t = 0, first = first0, rows = 0;
    while (t < n)
    {
      const size_t k = rnd_in(1, std::min<size_t>(n - t, 700));
      const size_t r = power_sum_rows(k, every, first);
      CHECK(r >= 1, "a call with samples writes a row");
      // the head of a later call completes the previous call's last row, unless the call starts on a grid point
      const bool head_joins = t > 0 && first > 0;
      rows += r - (head_joins ? 1 : 0);
      const size_t nf = every_next_first(k, every, first);
      // the grid goes on where it left off: the next grid point at or after t + k, relative to t + k
      size_t g = first0;
      while (g < t + k) g += every;
      CHECK(nf == g - (t + k), "t %zu k %zu every %zu first %zu: next first %zu, the grid says %zu", t, k, every, first, nf, g - (t + k));
      t += k; first = nf;
    }
    CHECK(rows == whole, "n %zu every %zu first %zu: %zu rows from the calls, %zu from one call", n, every, first0, rows, whole);
  }
}

int main()
{
  test_route();
  test_workspace();
  test_segments();
  test_rows_and_next_first();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("lag-sum-logic: all properties hold\n");
  return 0;
}
