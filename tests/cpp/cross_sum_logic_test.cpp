// cross_sum_logic_test.cpp -- the host-side decisions of the pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n) in
// sdft_plan_logic.hpp: which pair lists are accepted, the table of work items a pair list becomes (one item per pair, one
// advance-only item per channel no pair names, one writer per channel), the workspace and its slots, the time chunks and the route.
// Compiled by tests/test_cross_sum_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
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

static long checked = 0;

// every property the kernel and the plan rely on, for one accepted list
static void check_items(size_t channels, const std::vector<size_t>& a, const std::vector<size_t>& b)
{
  const size_t np = a.size();
  CHECK(cross_pairs_check(channels, np, a.data(), b.data()) == CX_OK, "%zu channels, %zu pairs: refused", channels, np);
  const std::vector<CrossItem> items = cross_items(channels, np, a.data(), b.data());
  ++checked;
  std::vector<int> writers(channels, 0), named(channels, 0), advance(channels, 0), outs(np, 0);
  for (size_t p = 0; p < np; ++p) { named[a[p]] = 1; named[b[p]] = 1; }
  CHECK(items.size() >= np && items.size() <= np + channels, "%zu items for %zu pairs of %zu channels", items.size(), np, channels);
  for (size_t i = 0; i < items.size(); ++i)
  {
    const CrossItem& it = items[i];
    CHECK(it.a < channels && it.b < channels, "item %zu names channel %u / %u of %zu", i, it.a, it.b, channels);
    if (it.a >= channels || it.b >= channels) return;
    CHECK(it.writes_a <= 1 && it.writes_b <= 1, "item %zu: flags", i);
    if (it.out == kCrossNone)
    {
      // advance-only: one channel, which no pair names, after all the pairs' items, and it is that channel's writer
      CHECK(it.a == it.b && !named[it.a], "item %zu advances channel %u, which a pair names", i, it.a);
      CHECK(i >= np, "item %zu: an advance-only item among the pairs' items", i);
      CHECK(it.writes_a == 1 && it.writes_b == 0, "item %zu: an advance-only item writes its channel on side a", i);
      ++advance[it.a];
    }
    else
    {
      // the item of pair p sits at index p: the workspace of item i is the workspace of pair i
      CHECK(it.out >= 0 && (size_t)it.out < np && (size_t)it.out == i, "item %zu forms pair %d", i, it.out);
      if (it.out < 0 || (size_t)it.out >= np) return;
      CHECK(it.a == a[it.out] && it.b == b[it.out], "item %zu: (%u, %u) for pair (%zu, %zu)", i, it.a, it.b, a[it.out], b[it.out]);
      ++outs[it.out];
      if (it.a == it.b) CHECK(it.writes_b == 0, "item %zu: a == b is written from side a only", i);
    }
    writers[it.a] += it.writes_a;
    writers[it.b] += it.writes_b;
  }
  for (size_t p = 0; p < np; ++p) CHECK(outs[p] == 1, "pair %zu has %d items", p, outs[p]);
  for (size_t c = 0; c < channels; ++c)
  {
    CHECK(writers[c] == 1, "channel %zu of %zu has %d writers (%zu pairs)", c, channels, writers[c], np);
    CHECK(advance[c] == (named[c] ? 0 : 1), "channel %zu: %d advance-only items, named %d", c, advance[c], named[c]);
  }
}

static void test_items()
{
  // exhaustive: up to 4 channels, lists of up to 3 pairs (the empty list too: every channel advances)
  for (size_t channels = 1; channels <= 4; ++channels)
    for (size_t np = 0; np <= 3; ++np)
    {
      const size_t per = channels * channels;
      size_t lists = 1;
      for (size_t p = 0; p < np; ++p) lists *= per;
      for (size_t code = 0; code < lists; ++code)
      {
        std::vector<size_t> a(np), b(np);
        size_t c = code;
        for (size_t p = 0; p < np; ++p) { a[p] = (c % per) / channels; b[p] = (c % per) % channels; c /= per; }
        check_items(channels, a, b);
      }
    }
  // random lists for up to 64 channels
  for (int i = 0; i < 4000; ++i)
  {
    const size_t channels = rnd_in(1, 64), np = rnd_in(1, 200);
    const size_t top = rnd() & 1 ? channels - 1 : rnd_in(0, channels - 1);     // (lists that leave many channels unnamed, too)
    std::vector<size_t> a(np), b(np);
    for (size_t p = 0; p < np; ++p) { a[p] = rnd_in(0, top); b[p] = (rnd() % 4 == 0) ? a[p] : rnd_in(0, top); }
    check_items(channels, a, b);
  }
  // the rates script's list: 32 disjoint pairs of 64 channels -- 32 items, every side a writer
  {
    std::vector<size_t> a(32), b(32);
    for (size_t p = 0; p < 32; ++p) { a[p] = 2 * p; b[p] = 2 * p + 1; }
    const std::vector<CrossItem> items = cross_items(64, 32, a.data(), b.data());
    CHECK(items.size() == 32, "%zu items", items.size());
    for (const CrossItem& it : items) CHECK(it.writes_a == 1 && it.writes_b == 1, "disjoint pairs write both sides");
  }
  CHECK(checked == 5278 + 4000, "%ld lists", checked);
}

static void test_refusals()
{
  const size_t a[3] = {0, 1, 2}, b[3] = {2, 1, 0};
  CHECK(cross_pairs_check(3, 0, nullptr, nullptr) == CX_OK, "an empty list removes the installed one");
  CHECK(cross_pairs_check(3, 3, a, b) == CX_OK, "three pairs of three channels");
  CHECK(cross_pairs_check(3, 3, nullptr, b) == CX_NULL && cross_pairs_check(3, 3, a, nullptr) == CX_NULL, "NULL arrays");
  CHECK(cross_pairs_check(2, 3, a, b) == CX_CHANNEL, "channel 2 of 2");
  CHECK(cross_pairs_check(1, 1, a, a) == CX_OK && cross_pairs_check(1, 1, a, b) == CX_CHANNEL && cross_pairs_check(1, 1, b, a) == CX_CHANNEL,
        "a single-channel plan accepts (0, 0) only");
  CHECK(cross_pairs_check(0, 1, a, a) == CX_OK, "channels == 0 is a plan of one channel");
  CHECK(cross_pairs_check(3, ((size_t)1 << 31) + 1, a, b) == CX_TOO_MANY, "more than 2^31 pairs (refused before the arrays are read)");
  const size_t huge[1] = {(size_t)-1};
  CHECK(cross_pairs_check(64, 1, huge, a) == CX_CHANNEL && cross_pairs_check(64, 1, a, huge) == CX_CHANNEL, "an index no unsigned holds");
}

static void test_workspace()
{
  for (int i = 0; i < 20000; ++i)
  {
    const size_t items = rnd_in(1, 200), chunks = rnd_in(1, 900), nb = rnd_in(1, 4096);
    CHECK(cross_sum_workspace(items, chunks, nb) == power_sum_workspace(items, chunks, 2 * nb), "the pooled power call's workspace of 2 nbins_out numbers");
    CHECK(cross_sum_workspace(items, chunks, nb) == (chunks > 1 ? items * chunks * 2 * 2 * nb : 0), "[items][chunks][2][nbins_out] complex");
    const size_t item = rnd_in(0, items - 1), chunk = rnd_in(0, chunks - 1);
    for (int slot = 0; slot < 2; ++slot)
    {
      const size_t at = cross_sum_slot(item, chunks, chunk, slot, nb);
      CHECK(at == power_sum_slot(item, chunks, chunk, slot, 2 * nb), "the pooled power call's slot");
      CHECK(at == ((item * chunks + chunk) * 2 + (size_t)slot) * 2 * nb, "slot arithmetic");
      if (chunks > 1) CHECK(at + 2 * nb <= cross_sum_workspace(items, chunks, nb), "the slot lies inside the workspace");
    }
    CHECK(cross_sum_slot(item, chunks, chunk, kPowerSumTailSlot, nb) == cross_sum_slot(item, chunks, chunk, kPowerSumHeadSlot, nb) + 2 * nb, "tail after head");
    const size_t rows = rnd_in(1, 7000);
    CHECK(cross_pair_stride(rows, nb) == rows * 2 * nb, "numbers from pair to pair");
  }
}

static void test_route()
{
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery fq;
    fq.n = rnd_in(1, 2000000); fq.nbins = rnd_in(1, 4200); fq.channels = rnd_in(1, 64);
    const bool f32 = rnd() & 1;
    fq.fd_bytes = f32 ? 4 : 8; fq.fdx_bytes = f32 ? 8 : 16;
    fq.window = (int)rnd_in(0, 3); fq.cursor = rnd_in(0, 2 * fq.nbins - 1); fq.exact = f32 || (rnd() & 1); fq.fid_canonical = rnd() & 1;
    fq.cross_sum = true; fq.cross_items = rnd_in(1, 130);
    fq.analysis_batch = rnd() & 1; fq.pipe_wanted = rnd() & 1;
    if (rnd() % 4 == 0) fq.chunk = (long)rnd_in(1, 5000);
    if (rnd() % 4 == 0) fq.segments = (long)rnd_in(1, 5);
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_CROSS_SUM, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.prefix && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    CHECK(r.chunks >= 1 && r.segments >= 1 && r.segments <= r.chunks, "n %zu: %ld segments of %ld chunks", fq.n, r.segments, r.chunks);
    CHECK(r.chunks == 1 || (long)r.shift < r.len, "n %zu: chunks of %ld shifted by %ld", fq.n, r.len, (long)r.shift);
    // the chunk choice is the pooled power call's with the items in the channels' place
    EveryQuery e;
    e.n = fq.n; e.channels = fq.cross_items; e.tiles = tiles(fq.nbins, fq.window, fq.fdx_bytes, fq.interior); e.exact = fq.exact; e.forced_chunk = fq.chunk;
    e.compute_units = fq.compute_units;
    const Chunking c = choose_power_sum_chunks(e);
    CHECK(r.len == c.len && (r.shift ? r.chunks >= c.chunks : r.chunks == c.chunks), "n %zu: %ld chunks of %ld, the pooled power call of %zu channels has %ld of %ld",
          fq.n, r.chunks, r.len, fq.cross_items, c.chunks, c.len);
    // the pooled power call of a plan with that many channels: the same chunks
    ForwardQuery pq = fq; pq.cross_sum = false; pq.cross_items = 0; pq.power_sum = true; pq.channels = fq.cross_items; pq.chain = 2;
    ForwardQuery cq = fq; cq.chain = 2;
    const ForwardRoute rp = forward_route(pq, [] { return true; }), rc = forward_route(cq, [] { return true; });
    CHECK(rp.kernel == FK_POWER_SUM && rp.chunks == rc.chunks && rp.len == rc.len && rp.carry == rc.carry && rp.shift == rc.shift, "the pooled power call's route");
  }
  CHECK(FK_CROSS_SUM == 8, "get_option(\"last_kernel\") answers 8");
}

// The carry forms of the shapes tests/test_gpu_cross_sum_routes.py runs on the GPU (4 channels, the 6 pairs of PAIRS and one
// advance-only item, n = 6000): what its assertions on last_chain, last_segments and last_chunk_len rest on.
static ForwardQuery gpu_test_query(size_t nbins, bool f32, size_t n, size_t cursor)
{
  ForwardQuery q;
  q.n = n; q.nbins = nbins; q.channels = 4; q.fd_bytes = f32 ? 4 : 8; q.fdx_bytes = f32 ? 8 : 16;
  q.window = kWindowHann; q.cursor = cursor; q.exact = true; q.fid_canonical = true;
  q.cross_sum = true; q.cross_items = 7;
  return q;
}
static ForwardRoute route_of(const ForwardQuery& q)
{
  bool asked = false;
  const ForwardRoute r = forward_route(q, [&] { asked = true; return true; });
  CHECK(r.kernel == FK_CROSS_SUM && !r.flow && !asked, "N %zu: never the flow form", q.nbins);
  return r;
}
static void test_carry_forms()
{
  for (int f32 = 0; f32 < 2; ++f32)
  {
    // N = 125: no block length (8 ... 128) divides 2N = 250, so the exact carries are the serial pass whatever option chain says
    for (long chain : {0L, 1L, 2L})
      for (long chunk : {0L, 128L})
      {
        ForwardQuery q = gpu_test_query(125, f32, 6000, 0); q.chain = chain; q.chunk = chunk;
        const ForwardRoute r = route_of(q);
        CHECK(r.chunks > 1 && r.carry == CARRY_SERIAL && r.relay_L == 0 && r.shift == 0 && r.use_seed, "N 125, chain %ld, chunk %ld: carry %d, L %u", chain, chunk, r.carry, r.relay_L);
      }
    // N = 1000: the relay form by default, with chain = 2, with forced chunks and in forced segments; chunks begin on block boundaries
    for (long chain : {1L, 2L})
      for (long chunk : {0L, 128L, 1000L})
        for (long segments : {0L, 3L})
          for (size_t cursor : {(size_t)0, (size_t)700, (size_t)1500})
          {
            const size_t n = 6000 - cursor;
            ForwardQuery q = gpu_test_query(1000, f32, n, cursor); q.chain = chain; q.chunk = chunk; q.segments = segments;
            const ForwardRoute r = route_of(q);
            CHECK(r.carry == CARRY_RELAY && r.relay_L >= 8 && r.use_seed, "N 1000, chain %ld, chunk %ld, cursor %zu: carry %d", chain, chunk, cursor, r.carry);
            if (r.carry != CARRY_RELAY) continue;
            CHECK(2000 % r.relay_L == 0 && r.len % (long)r.relay_L == 0, "block %u, chunks of %ld", r.relay_L, r.len);
            CHECK(r.shift == cursor % r.relay_L && (cursor == 0) == (r.shift == 0), "cursor %zu, block %u: shift %u", cursor, r.relay_L, r.shift);
            CHECK(r.chunks > 1 && (size_t)r.chunks * (size_t)r.len >= n + r.shift && (size_t)(r.chunks - 1) * (size_t)r.len < n + r.shift, "%ld chunks of %ld for %zu + %u", r.chunks, r.len, n, r.shift);
            if (chunk) CHECK(r.len == chunk, "forced chunk %ld: %ld", chunk, r.len);
            if (segments) CHECK(r.segments == segments, "forced segments %ld: %ld", segments, r.segments);
          }
    // ... and the serial pass with chain = 0, and after sdft_hip_set_state (the fid is the host's: not the canonical rotation)
    for (int installed = 0; installed < 2; ++installed)
      for (size_t cursor : {(size_t)0, (size_t)1500})
      {
        ForwardQuery q = gpu_test_query(1000, f32, 6000 - cursor, cursor); q.chain = installed ? 1 : 0; q.fid_canonical = !installed;
        const ForwardRoute r = route_of(q);
        CHECK(r.chunks > 1 && r.carry == CARRY_SERIAL && r.relay_L == 0 && r.shift == 0 && r.use_seed, "N 1000, installed %d: carry %d", installed, r.carry);
      }
  }
  // FD double with its default carries: partial sums + scan, the fid from the closed-form table
  ForwardQuery q = gpu_test_query(125, false, 6000, 0); q.exact = false;
  const ForwardRoute r = route_of(q);
  CHECK(r.chunks > 1 && r.carry == CARRY_SUMS && !r.use_seed && r.segments == 1, "FD double, default carries: carry %d", r.carry);
  // the 70-pair list of 5 channels (70 items: every channel is named), N = 64, n = 3000, and the lists of two and three pairs
  for (size_t items : {(size_t)4, (size_t)3, (size_t)5, (size_t)70})
    for (int f32 = 0; f32 < 2; ++f32)
    {
      ForwardQuery w = gpu_test_query(64, f32, 3000, 0); w.channels = 5; w.cross_items = items; w.exact = f32;
      CHECK(route_of(w).chunks > 1, "%zu items, N 64, n 3000: one chunk", items);
    }
}

// how stage_bytes bounds the segments of the staging tests (band of 100 bins, 6 pairs, 4 channels of float samples)
static void test_stage_rows()
{
  for (size_t fd : {(size_t)4, (size_t)8})
  {
    const size_t row = 6 * 2 * 100 * fd;
    CHECK(stage_rows(6000, row, 7 * row) == 7 && stage_rows(6000, row, 2 * row) == 2, "7 and 2 rows of sums");
    CHECK(stage_rows(6000, row, 700 * 4 * 4) == (fd == 4 ? 2u : 1u), "700 samples' bytes hold %zu rows of sums", stage_rows(6000, row, 700 * 4 * 4));
  }
  CHECK(stage_rows(6000, 4 * 4, 700 * 4 * 4) == 700 && 700 > (size_t)kHopSamples, "700 samples of 4 channels: a segment bound by the samples' bytes");
  CHECK(stage_rows(6000, 4 * 4, 1) == 1 && stage_rows(5, 16, 1 << 30) == 5 && stage_rows(0, 16, 64) == 1, "at least one row, at most the call's");
}

int main()
{
  test_items();
  test_refusals();
  test_workspace();
  test_route();
  test_carry_forms();
  test_stage_rows();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("cross-sum-logic: all properties hold\n");
  return 0;
}
