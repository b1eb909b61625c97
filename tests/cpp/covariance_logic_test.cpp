// covariance_logic_test.cpp -- the host-side decisions of the array covariance analysis (sdft_hip_sdft_covariance_n) in
// sdft_plan_logic.hpp: which arrays are accepted, the index of an element of the upper triangle, the table of block items an
// array becomes for a group size G (every pair in exactly one slot pair of one block, the lower array index on side A, one state
// writer per channel, one advance-only item per channel outside the array), the workspace and the route.
// Compiled by tests/test_covariance_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated
// property.

#include "sdft_plan_logic.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
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

static long checked = 0;

// every property the kernel and the plan rely on, for one accepted array (chan == nullptr: the channels 0 ... nch - 1) and one G
static void check_items(size_t channels, size_t nch, const size_t* chan, int G)
{
  CHECK(array_check(channels, nch, chan) == AR_OK, "%zu channels, %zu in the array: refused", channels, nch);
  const std::vector<CovItem> items = covariance_items(channels, nch, chan, G);
  ++checked;
  const size_t T = covariance_pairs(nch), groups = (nch + (size_t)G - 1) / (size_t)G;
  std::vector<int> produced(T, 0), writers(channels, 0), advanced(channels, 0), in_array(channels, 0);
  for (size_t i = 0; i < nch; ++i) in_array[chan ? chan[i] : i] = 1;
  CHECK(items.size() == groups * (groups + 1) / 2 + (channels - nch), "%zu items for %zu groups and %zu channels outside", items.size(), groups, channels - nch);
  bool past_blocks = false;
  for (size_t n = 0; n < items.size(); ++n)
  {
    const CovItem& it = items[n];
    if (!it.block)
    {
      // advance-only: one plan channel outside the array, after all blocks, and it is that channel's writer
      past_blocks = true;
      CHECK(it.a0 < channels && it.a0 == it.b0 && it.na == 1 && it.nb == 0 && it.writes == 1, "item %zu: advance-only form", n);
      if (it.a0 >= channels) return;
      CHECK(!in_array[it.a0], "item %zu advances channel %u, which is in the array", n, it.a0);
      ++advanced[it.a0]; ++writers[it.a0];
      for (size_t sa = 0; sa < 8; ++sa)
        for (size_t sb = 0; sb < 8; ++sb) CHECK(covariance_item_out(nch, it, sa, sb) == -1, "item %zu: an advance-only item forms a pair", n);
      continue;
    }
    CHECK(!past_blocks, "item %zu: a block after an advance-only item", n);
    CHECK(it.a0 <= it.b0 && it.a0 % (unsigned)G == 0 && it.b0 % (unsigned)G == 0, "item %zu: groups start at %u and %u", n, it.a0, it.b0);
    CHECK(it.na >= 1 && it.na <= G && it.nb >= 1 && it.nb <= G && it.a0 + it.na <= nch && it.b0 + it.nb <= nch, "item %zu: sides of %u and %u", n, it.na, it.nb);
    CHECK(it.na == std::min<size_t>((size_t)G, nch - it.a0) && it.nb == std::min<size_t>((size_t)G, nch - it.b0), "item %zu: a side is not its whole group", n);
    CHECK((it.writes != 0) == (it.a0 == it.b0), "item %zu: the diagonal blocks, and only they, write", n);
    if (it.a0 + it.na > nch || it.b0 + it.nb > nch) return;
    if (it.writes)
      for (size_t s = 0; s < it.na; ++s) ++writers[chan ? chan[it.a0 + s] : it.a0 + s];
    for (size_t sa = 0; sa < (size_t)G + 1; ++sa)
      for (size_t sb = 0; sb < (size_t)G + 1; ++sb)
      {
        const long out = covariance_item_out(nch, it, sa, sb);
        const bool forms = sa < it.na && sb < it.nb && (it.a0 != it.b0 || sa <= sb);
        CHECK((out >= 0) == forms, "item %zu slots (%zu, %zu): out %ld", n, sa, sb, out);
        if (out < 0) continue;
        const size_t i = it.a0 + sa, j = it.b0 + sb;
        CHECK(i <= j, "item %zu slots (%zu, %zu): side A holds array index %zu, side B %zu", n, sa, sb, i, j);
        CHECK((size_t)out < T && (size_t)out == covariance_pair_index(nch, i, j), "item %zu slots (%zu, %zu): index %ld", n, sa, sb, out);
        if ((size_t)out < T) ++produced[out];
      }
  }
  for (size_t p = 0; p < T; ++p) CHECK(produced[p] == 1, "nch %zu G %d: element %zu is produced %d times", nch, G, p, produced[p]);
  for (size_t c = 0; c < channels; ++c)
  {
    CHECK(writers[c] == 1, "channel %zu of %zu has %d writers (nch %zu, G %d)", c, channels, writers[c], nch, G);
    CHECK(advanced[c] == (in_array[c] ? 0 : 1), "channel %zu: %d advance-only items, in the array %d", c, advanced[c], in_array[c]);
  }
}

int main()
{
  // the index formula: a bijection of the upper triangle onto 0 ... T - 1, in row-major order
  for (size_t nch = 1; nch <= 70; ++nch)
  {
    size_t next = 0;
    for (size_t i = 0; i < nch; ++i)
      for (size_t j = i; j < nch; ++j) { CHECK(covariance_pair_index(nch, i, j) == next, "nch %zu (%zu, %zu)", nch, i, j); ++next; }
    CHECK(next == covariance_pairs(nch), "nch %zu: %zu elements", nch, next);
  }
  CHECK(covariance_pair_index(kArrayMaxChannels, kArrayMaxChannels - 1, kArrayMaxChannels - 1) + 1 == covariance_pairs(kArrayMaxChannels) &&
        covariance_pairs(kArrayMaxChannels) < ((size_t)1 << 31), "the largest array's pairs fit 31 bits");

  // item tables: every channels 1 ... 9, every nch, the identity list (given and as nullptr), permuted lists and subsets
  for (size_t channels = 1; channels <= 9; ++channels)
    for (size_t nch = 1; nch <= channels; ++nch)
      for (int G : {1, 2, 4, 8})
      {
        check_items(channels, nch, nullptr, G);
        std::vector<size_t> all(channels);
        std::iota(all.begin(), all.end(), (size_t)0);
        check_items(channels, nch, all.data(), G);                       // (the first nch channels)
        for (int trial = 0; trial < 6; ++trial)
        {
          std::vector<size_t> perm = all;
          for (size_t i = channels - 1; i > 0; --i) std::swap(perm[i], perm[(size_t)(rnd() % (i + 1))]);
          check_items(channels, nch, perm.data(), G);                    // a permuted subset of nch channels
        }
      }

  // refused lists leave nothing to build
  {
    const size_t twice[3] = {1, 2, 1}, far[2] = {0, 5}, ok[3] = {4, 0, 2};
    CHECK(array_check(5, 3, twice) == AR_REPEAT, "a repeated channel");
    CHECK(array_check(5, 2, far) == AR_CHANNEL, "a channel the plan does not have");
    CHECK(array_check(5, 6, nullptr) == AR_TOO_MANY && array_check(2, 3, ok) == AR_TOO_MANY, "more channels than the plan has");
    CHECK(array_check(5, 3, ok) == AR_OK && array_check(5, 5, nullptr) == AR_OK && array_check(5, 0, nullptr) == AR_OK, "accepted lists");
    CHECK(array_check(1, 1, nullptr) == AR_OK && array_check(0, 1, nullptr) == AR_OK, "a single-channel plan has the array {0}");
    const size_t zero[1] = {0}, one[1] = {1};
    CHECK(array_check(1, 1, zero) == AR_OK && array_check(1, 1, one) == AR_CHANNEL, "a single-channel plan");
    CHECK(array_check((size_t)1 << 20, kArrayMaxChannels + 1, nullptr) == AR_TOO_MANY, "more pairs than 32 bits count");
  }

  // the workspace is the cross-spectrum call's with T pairs, slot by output index
  for (size_t nch : {1u, 2u, 5u, 9u, 64u})
    for (size_t chunks : {1u, 2u, 7u})
      for (size_t nb : {1u, 125u, 1024u})
      {
        const size_t T = covariance_pairs(nch);
        CHECK(covariance_workspace(nch, chunks, nb) == cross_sum_workspace(T, chunks, nb), "workspace");
        if (chunks > 1) CHECK(cross_sum_slot(T - 1, chunks, chunks - 1, kPowerSumTailSlot, nb) + 2 * nb == covariance_workspace(nch, chunks, nb), "the last slot ends the workspace");
      }

  // the route: kernel 9, the grid kernels' tile form, the block items in the channels' place when time is cut
  {
    ForwardQuery q;
    q.n = 48000; q.nbins = 1024; q.channels = 64; q.fd_bytes = 8; q.fdx_bytes = 16;
    q.covariance = true;
    const size_t few = covariance_items(64, 64, nullptr, 4).size(), many = covariance_items(64, 64, nullptr, 1).size();
    CHECK(few == 136 && many == 2080, "items of 64 channels: %zu at G = 4, %zu at G = 1", few, many);
    q.cross_items = few;
    const ForwardRoute r4 = forward_route(q, [] { return false; });
    q.cross_items = many;
    const ForwardRoute r1 = forward_route(q, [] { return false; });
    CHECK(r4.kernel == FK_COVARIANCE && r1.kernel == FK_COVARIANCE && FK_COVARIANCE == 9, "last_kernel");
    CHECK(!r4.pipelined && !r4.self && !r4.prefix && !r4.flow && !r4.fused, "never pipelined, self-carried or fused");
    CHECK(r4.chunks > r1.chunks && r1.chunks >= 1, "fewer items, more chunks: %ld against %ld", r4.chunks, r1.chunks);
    // the same query as a cross-spectrum call of as many items is cut the same way (choose_power_sum_chunks)
    ForwardQuery c = q;
    c.covariance = false; c.cross_sum = true; c.cross_items = few;
    const ForwardRoute rc = forward_route(c, [] { return false; });
    CHECK(rc.chunks == r4.chunks && rc.len == r4.len && rc.kernel == FK_CROSS_SUM, "the cross-spectrum call's chunks");
    q.n = 500; q.cross_items = few;
    const ForwardRoute rs = forward_route(q, [] { return false; });
    CHECK(rs.chunks == 1 && rs.kernel == FK_COVARIANCE, "a call shorter than 512 samples is one chunk of the covariance kernel");
  }

  if (failures) { fprintf(stderr, "covariance-logic: %d properties violated\n", failures); return 1; }
  printf("covariance-logic: all properties hold (%ld item tables)\n", checked);
  return 0;
}
