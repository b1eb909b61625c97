// power_sum_logic_test.cpp -- the host-side decisions of the pooled power analysis (sdft_hip_sdft_power_sum_n) in
// sdft_plan_logic.hpp: the row count, the window of a sample and of a row, what a time chunk does with its windows (whole rows,
// head and tail pieces, workspace slots), the chunks whose pieces make a row, the streaming identity, the time chunks and the route.
// Compiled by tests/test_power_sum_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <utility>
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

// the windows of a call by direct enumeration: walk the samples, a new window at sample 0 and at every grid point
typedef std::vector<std::pair<size_t, size_t>> Windows;      // [begin, end) per row
static Windows brute_windows(size_t n, size_t every, size_t first)
{
  Windows w;
  for (size_t t = 0; t < n; ++t)
  {
    const bool grid = t >= first && (t - first) % every == 0;
    if (t == 0 || grid) w.push_back({t, t + 1});
    else w.back().second = t + 1;
  }
  return w;
}

struct Case { size_t n, every, first; };
static std::vector<Case> cases()
{
  std::vector<Case> c;
  for (size_t n = 0; n <= 40; ++n)
    for (size_t every = 1; every <= 12; ++every)
      for (size_t first = 0; first <= 14; ++first) c.push_back({n, every, first});
  // every >= n, first >= n, both
  const Case more[] = {{30, 30, 0}, {30, 31, 0}, {30, 1000, 0}, {30, 1000, 7}, {30, 5, 30}, {30, 5, 31}, {30, 5, 7000}, {30, 64, 64},
                       {1, 1, 0}, {1, 1, 1}, {1, 9, 5}, {40, 40, 39}, {40, 41, 40}, {37, (size_t)1 << 40, 3}, {37, 3, (size_t)1 << 40}};
  for (const Case& m : more) c.push_back(m);
  return c;
}

static void test_rows_and_windows()
{
  for (const Case& k : cases())
  {
    const Windows w = brute_windows(k.n, k.every, k.first);
    CHECK(power_sum_rows(k.n, k.every, k.first) == w.size(), "n %zu every %zu first %zu: %zu rows, enumerated %zu", k.n, k.every, k.first,
          power_sum_rows(k.n, k.every, k.first), w.size());
    CHECK(power_sum_rows(k.n, k.every, k.first) == (k.first > 0 && k.n > 0 ? 1 : 0) + every_rows(k.n, k.every, k.first), "the issue's formula");
    CHECK((power_sum_rows(k.n, k.every, k.first) == 0) == (k.n == 0), "0 rows only for an empty call");
    for (size_t r = 0; r < w.size(); ++r)
    {
      const PowerSumWindow rw = power_sum_row_window(r, k.n, k.every, k.first);
      CHECK(rw.row == r && rw.begin == w[r].first && rw.end == w[r].second, "n %zu every %zu first %zu row %zu: [%zu, %zu), enumerated [%zu, %zu)",
            k.n, k.every, k.first, r, rw.begin, rw.end, w[r].first, w[r].second);
      for (size_t t = w[r].first; t < w[r].second; ++t)
      {
        const PowerSumWindow sw = power_sum_window(t, k.n, k.every, k.first);
        CHECK(sw.row == r && sw.begin == w[r].first && sw.end == w[r].second, "n %zu every %zu first %zu sample %zu: row %zu, enumerated %zu", k.n, k.every,
              k.first, t, sw.row, r);
      }
    }
  }
  CHECK(power_sum_rows(1000000, 1, 0) == 1000000 && power_sum_rows(1000000, 1000000, 0) == 1 && power_sum_rows(6000, 50, 7000) == 1, "examples");
  CHECK(power_sum_rows(6000, 100, 37) == 61 && power_sum_rows(6000, 10000, 0) == 1 && power_sum_rows(0, 5, 3) == 0, "examples");
}

// every chunk length and shift the chunk rule can produce on calls this short: any length from 1 to n (forced chunks, exact or
// not), any shift below the length (the ring form moves every chunk but the first down by less than a chunk)
static void test_chunks_and_pieces()
{
  size_t walked = 0;
  for (const Case& k : cases())
  {
    if (k.n == 0) continue;
    const Windows w = brute_windows(k.n, k.every, k.first);
    for (long len = 1; len <= (long)k.n; ++len)
      for (long shift = 0; shift < len; shift += (len > 8 ? 3 : 1))
      {
        long chunks = 0;
        while (chunk_begin(chunks, len, shift) < k.n) ++chunks;
        ++walked;
        // sample -> (chunk, row) by enumeration; every sample in exactly one chunk, found by chunk_of
        std::vector<int> seen(k.n, 0);
        // what lands where: slots and rows written, with the samples they hold
        std::map<std::pair<long, int>, std::pair<size_t, size_t>> slot;          // (chunk, slot) -> [begin, end)
        std::map<size_t, long> whole;                                              // row -> chunk that stores it
        for (long c = 0; c < chunks; ++c)
        {
          const size_t t0 = chunk_begin(c, len, shift), t1 = chunk_end(c, len, shift, k.n);
          CHECK(t0 < t1 && t1 <= k.n, "chunk %ld of %ld: [%zu, %zu)", c, chunks, t0, t1);
          for (size_t t = t0; t < t1; ++t) { ++seen[t]; CHECK(chunk_of(t, len, shift) == c, "sample %zu: chunk %ld, not %ld", t, chunk_of(t, len, shift), c); }
          const PowerSumChunk p = power_sum_chunk(t0, t1, k.n, k.every, k.first);
          // the chunk's samples, window by window, against p
          size_t covered = 0;
          if (p.head)
          {
            const auto& win = w[p.head_row];
            CHECK(win.first < t0 && win.second > t0, "head piece of a window that does not cross t0");
            slot[{c, kPowerSumHeadSlot}] = {t0, std::min(win.second, t1)};
            covered += std::min(win.second, t1) - t0;
          }
          for (size_t r = p.whole_row0; r < p.whole_row0 + p.whole_rows; ++r)
          {
            CHECK(r < w.size() && w[r].first >= t0 && w[r].second <= t1, "row %zu is not whole in chunk %ld", r, c);
            CHECK(!whole.count(r), "row %zu stored twice", r);
            whole[r] = c;
            if (r < w.size()) covered += w[r].second - w[r].first;
          }
          if (p.tail)
          {
            const auto& win = w[p.tail_row];
            CHECK(win.first >= t0 && win.first < t1 && win.second > t1, "tail piece of a window that does not begin in the chunk and cross t1");
            slot[{c, kPowerSumTailSlot}] = {win.first, t1};
            covered += t1 - win.first;
          }
          CHECK(covered == t1 - t0, "n %zu every %zu first %zu len %ld shift %ld chunk %ld: %zu of %zu samples in a piece", k.n, k.every, k.first, len, shift,
                c, covered, t1 - t0);
          CHECK(!(p.head && p.tail && p.head_row == p.tail_row), "one window, two slots");
        }
        for (size_t t = 0; t < k.n; ++t) CHECK(seen[t] == 1, "sample %zu in %d chunks", t, seen[t]);
        // slots of the workspace are distinct and inside it
        {
          std::set<size_t> offsets;
          const size_t nb = 3, channels = 2;
          for (size_t ch = 0; ch < channels; ++ch)
            for (long c = 0; c < chunks; ++c)
              for (int s = 0; s < 2; ++s)
              {
                const size_t o = power_sum_slot(ch, (size_t)chunks, (size_t)c, s, nb);
                CHECK(chunks == 1 || o + nb <= power_sum_workspace(channels, (size_t)chunks, nb), "slot past the workspace");
                CHECK(o % nb == 0 && offsets.insert(o).second, "two pieces share a slot");
              }
          CHECK(power_sum_workspace(channels, 1, nb) == 0, "one chunk cuts nothing");
        }
        // every row: whole in one chunk, or the pieces of its chunks in ascending order cover its window once
        for (size_t r = 0; r < w.size(); ++r)
        {
          const PowerSumWindow rw = power_sum_row_window(r, k.n, k.every, k.first);
          const PowerSumRowChunks rc = power_sum_row_chunks(rw, len, shift);
          CHECK(rc.c0 <= rc.c1 && rc.c1 < chunks, "row %zu: chunks %ld ... %ld of %ld", r, rc.c0, rc.c1, chunks);
          if (rc.c0 == rc.c1)
          {
            CHECK(whole.count(r) && whole[r] == rc.c0, "row %zu is whole in chunk %ld but that chunk does not store it", r, rc.c0);
            continue;
          }
          CHECK(!whole.count(r), "row %zu is cut and stored by a forward wave as well", r);
          size_t at = rw.begin;
          for (long c = rc.c0; c <= rc.c1; ++c)
          {
            const auto it = slot.find({c, c == rc.c0 ? kPowerSumTailSlot : kPowerSumHeadSlot});
            CHECK(it != slot.end(), "row %zu: chunk %ld has no piece", r, c);
            if (it == slot.end()) break;
            CHECK(it->second.first == at && it->second.second > at, "row %zu: piece of chunk %ld is [%zu, %zu), expected to start at %zu", r, c,
                  it->second.first, it->second.second, at);
            at = it->second.second;
            slot.erase(it);
          }
          CHECK(at == rw.end, "row %zu: pieces end at %zu, the window at %zu", r, at, rw.end);
        }
        CHECK(slot.empty(), "n %zu every %zu first %zu len %ld shift %ld: %zu pieces belong to no row", k.n, k.every, k.first, len, shift, slot.size());
      }
  }
  CHECK(walked > 100000, "%zu chunkings walked", walked);
}

// cutting [0, n) at any point, the second call with every_next_first: the rows of the two calls, the second's head added to the
// first's last row, are the windows of the one call
static void test_streaming()
{
  for (const Case& k : cases())
  {
    if (k.first > ((size_t)1 << 30) || k.every > ((size_t)1 << 30)) continue;      // (sample offsets below stay small)
    const Windows one = brute_windows(k.n, k.every, k.first);
    for (size_t cut = 0; cut <= k.n; ++cut)
    {
      const size_t f2 = every_next_first(cut, k.every, k.first);
      const size_t r1 = power_sum_rows(cut, k.every, k.first), r2 = power_sum_rows(k.n - cut, k.every, f2);
      Windows joined;
      for (size_t r = 0; r < r1; ++r) { const PowerSumWindow w = power_sum_row_window(r, cut, k.every, k.first); joined.push_back({w.begin, w.end}); }
      for (size_t r = 0; r < r2; ++r)
      {
        const PowerSumWindow w = power_sum_row_window(r, k.n - cut, k.every, f2);
        const bool head = r == 0 && f2 > 0 && cut > 0;
        if (head)
        {
          CHECK(!joined.empty() && joined.back().second == cut + w.begin, "the head does not continue the last row");
          if (!joined.empty()) joined.back().second = cut + w.end;
        }
        else joined.push_back({cut + w.begin, cut + w.end});
      }
      CHECK(joined == one, "n %zu every %zu first %zu cut at %zu (next first %zu): %zu rows after joining, %zu in one call", k.n, k.every, k.first, cut, f2,
            joined.size(), one.size());
    }
  }
}

static void test_chunk_choice_and_route()
{
  EveryQuery q;
  q.n = 1000000; q.channels = 1; q.tiles = 19; q.compute_units = 256;                 // configs[1]: N = 1024 double, Hann
  Chunking c = choose_power_sum_chunks(q);
  CHECK(c.len == 1160 && c.chunks == 863, "configs[1]: %ld chunks of %ld", c.chunks, c.len);
  q.n = 600;
  c = choose_power_sum_chunks(q);
  CHECK(c.len == 72 && c.chunks == 9, "a short call is cut at the dense minimum: %ld chunks of %ld", c.chunks, c.len);
  q.n = 511;
  c = choose_power_sum_chunks(q);
  CHECK(c.chunks == 1 && c.len == 511, "calls below kHopSamples are one chunk");
  for (int i = 0; i < 20000; ++i)
  {
    q.n = rnd_in(1, 3000000); q.channels = rnd_in(1, 64); q.tiles = (long)rnd_in(1, 80); q.exact = rnd() & 1;
    q.compute_units = (int)rnd_in(1, 304); q.forced_chunk = (rnd() % 4 == 0) ? (long)rnd_in(1, 5000) : 0;
    c = choose_power_sum_chunks(q);
    const Chunking dense = choose_power_chunks(q, 1);
    CHECK(c.len == dense.len && c.chunks == dense.chunks, "the dense power call's chunks");
    CHECK((size_t)(c.chunks - 1) * (size_t)c.len < q.n && (size_t)c.chunks * (size_t)c.len >= q.n, "n %zu: %ld chunks of %ld cover the call once", q.n, c.chunks, c.len);
  }
  for (int i = 0; i < 20000; ++i)
  {
    ForwardQuery fq;
    fq.n = rnd_in(1, 2000000); fq.nbins = rnd_in(1, 4200); fq.channels = rnd_in(1, 8);
    const bool f32 = rnd() & 1;
    fq.fd_bytes = f32 ? 4 : 8; fq.fdx_bytes = f32 ? 8 : 16;
    fq.window = (int)rnd_in(0, 3); fq.cursor = rnd_in(0, 2 * fq.nbins - 1); fq.exact = f32 || (rnd() & 1); fq.fid_canonical = rnd() & 1;
    fq.power_sum = true;
    fq.analysis_batch = rnd() & 1; fq.pipe_wanted = rnd() & 1;
    bool asked = false;
    const ForwardRoute r = forward_route(fq, [&] { asked = true; return true; });
    CHECK(r.kernel == FK_POWER_SUM, "n %zu N %zu: kernel %d", fq.n, fq.nbins, r.kernel);
    CHECK(!r.self && !r.flow && !r.pipelined && !r.fused && !r.rows_f32 && !r.arm_flag && !asked, "n %zu N %zu: a form the kernel does not have", fq.n, fq.nbins);
    CHECK(r.chunks >= 1 && r.segments >= 1 && r.segments <= r.chunks, "n %zu: %ld segments of %ld chunks", fq.n, r.segments, r.chunks);
    CHECK(r.chunks == 1 || (long)r.shift < r.len, "n %zu: chunks of %ld shifted by %ld", fq.n, r.len, (long)r.shift);
    // the dense power call of the same shape: the same chunks and carries
    ForwardQuery pq = fq; pq.power_sum = false; pq.power = true; pq.power_every = 1;
    const ForwardRoute rp = forward_route(pq, [] { return true; });
    CHECK(rp.kernel == FK_POWER && rp.chunks == r.chunks && rp.len == r.len && rp.carry == r.carry && rp.relay_L == r.relay_L && rp.shift == r.shift,
          "the dense power call's route");
  }
  CHECK(FK_POWER_SUM == 6, "get_option(\"last_kernel\") answers 6");
}

int main()
{
  test_rows_and_windows();
  test_chunks_and_pieces();
  test_streaming();
  test_chunk_choice_and_route();
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("power-sum-logic: all properties hold\n");
  return 0;
}
