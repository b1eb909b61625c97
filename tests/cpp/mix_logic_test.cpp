// mix_logic_test.cpp -- the host-side decisions of the channel-mix analysis (sdft_hip_sdft_mix_n) in sdft_plan_logic.hpp: which
// mixes are accepted, the table of items a mix becomes for a block size O (every output in exactly one block, one state writer per
// channel, one advance-only item per channel outside the mix), the layout of outputs and weights, and the route.
// Compiled by tests/test_mix_cpu.py with g++ -fsanitize=address,undefined (no HIP).  Exits non-zero at the first violated property.

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

// every property the kernel and the plan rely on, for one accepted mix (chan == nullptr: the channels 0 ... nch - 1) and one O
static void check_items(size_t channels, size_t nch, const size_t* chan, size_t nout, int O)
{
  CHECK(mix_check(channels, nout, nch, chan, true) == MX_OK, "%zu channels, %zu in the mix, %zu outputs: refused", channels, nch, nout);
  const std::vector<MixItem> items = mix_items(channels, nch, chan, nout, O);
  ++checked;
  const size_t blocks = (nout + (size_t)O - 1) / (size_t)O;
  std::vector<int> produced(nout, 0), writers(channels, 0), advanced(channels, 0), in_mix(channels, 0);
  for (size_t i = 0; i < nch; ++i) in_mix[chan ? chan[i] : i] = 1;
  CHECK(items.size() == blocks + (channels - nch), "%zu items for %zu blocks and %zu channels outside", items.size(), blocks, channels - nch);
  bool past_blocks = false;
  for (size_t n = 0; n < items.size(); ++n)
  {
    const MixItem& it = items[n];
    if (it.no == 0)
    {
      // advance-only: one plan channel outside the mix, after all blocks, and it is that channel's writer
      past_blocks = true;
      CHECK(it.o0 < channels && it.writes == 1, "item %zu: advance-only form", n);
      if (it.o0 >= channels) return;
      CHECK(!in_mix[it.o0], "item %zu advances channel %u, which is in the mix", n, it.o0);
      ++advanced[it.o0]; ++writers[it.o0];
      continue;
    }
    CHECK(!past_blocks, "item %zu: a block after an advance-only item", n);
    CHECK(it.o0 == n * (size_t)O && it.no <= O && it.o0 + it.no <= nout, "item %zu: outputs %u ... + %u", n, it.o0, it.no);
    CHECK(it.no == std::min<size_t>((size_t)O, nout - it.o0), "item %zu: not its whole block", n);
    CHECK((it.writes != 0) == (it.o0 == 0), "item %zu: the block of output 0, and only it, writes", n);
    if (it.o0 + it.no > nout) return;
    for (size_t o = 0; o < it.no; ++o) ++produced[it.o0 + o];
    if (it.writes)
      for (size_t i = 0; i < nch; ++i) ++writers[chan ? chan[i] : i];         // (a block steps every element of the mix)
  }
  for (size_t o = 0; o < nout; ++o) CHECK(produced[o] == 1, "nout %zu O %d: output %zu is produced %d times", nout, O, o, produced[o]);
  for (size_t c = 0; c < channels; ++c)
  {
    CHECK(writers[c] == 1, "channel %zu of %zu has %d writers (nch %zu, nout %zu, O %d)", c, channels, writers[c], nch, nout, O);
    CHECK(advanced[c] == (in_mix[c] ? 0 : 1), "channel %zu: %d advance-only items, in the mix %d", c, advanced[c], in_mix[c]);
  }
}

int main()
{
  // item tables: 9 channels and fewer, every nch, nout up to 5, every block size; the identity list (given and as nullptr),
  // permuted lists and subsets
  for (size_t channels = 1; channels <= 9; ++channels)
    for (size_t nch = 1; nch <= channels; ++nch)
      for (size_t nout = 1; nout <= 5; ++nout)
        for (int O : {1, 2, 4})
        {
          check_items(channels, nch, nullptr, nout, O);
          std::vector<size_t> all(channels);
          std::iota(all.begin(), all.end(), (size_t)0);
          check_items(channels, nch, all.data(), nout, O);                 // (the first nch channels)
          for (int trial = 0; trial < 3; ++trial)
          {
            std::vector<size_t> perm = all;
            for (size_t i = channels - 1; i > 0; --i) std::swap(perm[i], perm[(size_t)(rnd() % (i + 1))]);
            check_items(channels, nch, perm.data(), nout, O);              // a permuted subset of nch channels
          }
        }

  // accepted and refused mixes
  {
    const size_t twice[3] = {1, 2, 1}, far[2] = {0, 5}, ok[3] = {4, 0, 2};
    CHECK(mix_check(5, 2, 3, twice, true) == MX_REPEAT, "a repeated channel");
    CHECK(mix_check(5, 2, 2, far, true) == MX_CHANNEL, "a channel the plan does not have");
    CHECK(mix_check(5, 2, 6, nullptr, true) == MX_TOO_MANY && mix_check(2, 1, 3, ok, true) == MX_TOO_MANY, "more channels than the plan has");
    CHECK(mix_check(5, 2, 3, ok, false) == MX_NO_WEIGHTS && mix_check(5, 1, 5, nullptr, false) == MX_NO_WEIGHTS, "no weights");
    CHECK(mix_check(5, 2, 0, nullptr, true) == MX_NO_CHANNELS && mix_check(5, 2, 0, ok, true) == MX_NO_CHANNELS, "no channels");
    CHECK(mix_check(5, kMixMaxOutputs + 1, 3, ok, true) == MX_TOO_MANY_OUTPUTS && mix_check(5, kMixMaxOutputs, 3, ok, true) == MX_OK, "the most outputs");
    CHECK(mix_check(5, 2, 3, ok, true) == MX_OK && mix_check(5, 1, 5, nullptr, true) == MX_OK, "accepted mixes");
    // nout == 0 removes the mix, whatever else is passed
    CHECK(mix_check(5, 0, 0, nullptr, false) == MX_OK && mix_check(5, 0, 9, twice, false) == MX_OK && mix_check(0, 0, 0, nullptr, true) == MX_OK, "removal");
    const size_t zero[1] = {0}, one[1] = {1};
    CHECK(mix_check(1, 3, 1, zero, true) == MX_OK && mix_check(1, 3, 1, one, true) == MX_CHANNEL && mix_check(0, 1, 1, nullptr, true) == MX_OK, "a single-channel plan");
  }

  // layout: outputs are dense [nout][rows][nbins] complex, weights [nout][nch][dftsize]
  CHECK(mix_output_stride(7, 100) == 1400 && mix_output_stride(0, 100) == 0, "numbers from one output to the next");
  CHECK(mix_weight_index(3, 125, 0, 0, 0) == 0 && mix_weight_index(3, 125, 1, 2, 124) == 2 * 3 * 125 - 1 && mix_weight_index(3, 125, 1, 0, 0) == 375, "weights");

  // the route: kernel 10, the grid kernels' tile form, the items in the channels' place when time is cut, the power call's chunks
  {
    ForwardQuery q;
    q.n = 48000; q.nbins = 1024; q.channels = 64; q.fd_bytes = 8; q.fdx_bytes = 16;
    q.mix = true;
    const size_t one = mix_items(64, 64, nullptr, 1, 4).size(), four = mix_items(64, 64, nullptr, 4, 1).size(), sub = mix_items(64, 16, nullptr, 4, 4).size();
    CHECK(one == 1 && four == 4 && sub == 1 + 48, "items of 64 channels: %zu, %zu, %zu", one, four, sub);
    for (size_t every : {(size_t)1, (size_t)100})
    {
      q.power_every = every;
      q.cross_items = one;
      const ForwardRoute r1 = forward_route(q, [] { return false; });
      q.cross_items = sub;
      const ForwardRoute rs = forward_route(q, [] { return false; });
      CHECK(r1.kernel == FK_MIX && rs.kernel == FK_MIX && FK_MIX == 10, "last_kernel");
      CHECK(!r1.pipelined && !r1.self && !r1.prefix && !r1.flow && !r1.fused, "never pipelined, self-carried or fused");
      CHECK(r1.chunks > rs.chunks && rs.chunks >= 1, "fewer items, more chunks: %ld against %ld", r1.chunks, rs.chunks);
      // a power call of as many channels as the mix has items is cut the same way (choose_power_chunks)
      ForwardQuery c = q;
      c.mix = false; c.power = true; c.cross_items = 0; c.channels = sub;
      const ForwardRoute rp = forward_route(c, [] { return false; });
      CHECK(rp.chunks == rs.chunks && rp.len == rs.len && rp.kernel == FK_POWER, "the power call's chunks");
    }
    q.n = 500; q.cross_items = one;
    const ForwardRoute rh = forward_route(q, [] { return false; });
    CHECK(rh.chunks == 1 && rh.kernel == FK_MIX, "a call shorter than 512 samples is one chunk of the mix kernel");
  }

  if (failures) { fprintf(stderr, "mix-logic: %d properties violated\n", failures); return 1; }
  printf("mix-logic: all properties hold (%ld item tables)\n", checked);
  return 0;
}
