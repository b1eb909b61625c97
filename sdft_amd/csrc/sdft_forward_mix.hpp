// sdft_forward_mix.hpp -- K1m: channel-mix analysis (sdft_hip_sdft_mix_n), per-bin weighted sums of the windowed bins of the
// channels of a mix on a row grid: Y_o[t][k] = sum over the elements i of W[o][i][k] * X_chan[i][t][k]
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_covariance.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// channels of a group and outputs of a block, per FD type (measured: profiles/mix_rates.txt).  A build with -DSDFT_HIP_TEST_HOOKS
// also holds the other candidates, for scripts/mix_rates.py (options "mix_group" and "mix_block").
template <typename FD> struct mix_group { static constexpr int value = 4; };
template <typename FD> struct mix_block { static constexpr int value = 4; };

// One work item of a mix call (logic::mix_items).  A block item (no != 0) forms the outputs o0 ... o0 + no - 1 from ALL elements
// of the mix; the block of output 0 is the one item that writes the state of the mix's channels back (writes != 0).  Another item
// (no == 0) only advances the PLAN channel o0, which is not in the mix, and writes its state.
struct MixItem
{
  unsigned o0;
  unsigned short no, writes;
};

// PowerArgs with complex rows, the mix in place of the channels: chan[i] is the plan channel of element i, bin k of row r of output
// o goes to out + o * out_stride + 2 * (r * nbins_out + (k - bin0)) as (re, im)
template <typename FD> struct MixArgs
{
  FD* out;                    // [nout][rows][nbins_out] complex, aligned to sizeof(FD) only
  size_t out_stride;          // FD numbers per output
  const cx<FD>* weights;      // [nout][nch][N]
  const MixItem* items;       // [nitems]
  const unsigned* chan;       // [nch]
  unsigned nitems, nch, nout;
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// forward_power_kernel's geometry, carry-in, grid and time loop with forward_covariance_kernel's groups of G channels.  A wave is
// (tile, chunk, item).  A block item takes the groups of the mix one after the other and re-runs the chunk's time loop for each
// from the group's carry-in: between grid samples it only advances the G recurrences, at a grid sample it steps them, windows each
// channel ONCE and continues the running sums of its (up to) O outputs with the group's terms
//   re = fl(fl(wr * yr) - fl(wi * yi))        im = fl(fl(wr * yi) + fl(wi * yr))
// in element order, each component by itself, in FD.  The first group starts every sum from -0 (-0 + x is x for every x) and
// stores it in the row; a later group first loads what THIS lane stored there (plain loads and stores of one thread to one address:
// program order), adds and stores again.  The sum of a row is therefore the sequential one over the elements 0 ... nch - 1 whatever
// G and O are, with no workspace and no second kernel.  A group at the mix's end with fewer than G channels is padded with the
// mix's last channel: a padded slot is stepped like the others (no guard in the hot loop) and has no state to write; its terms are
// skipped by a wave-uniform test at the grid sample (a zero weight would not do: -0 + fl(0 * y) is +0, and NaN for an infinite y).
// Weights apply after the window, to owned bins of the band only: a lane reads those of its bins per group into registers, mirror
// and halo lanes hold zeros and store nothing.  An item that forms no row in this tile (a tile outside the band, an advance-only
// item) steps the channels it writes one after the other, without windows; another block has nothing to do there.
template <typename FD, int BPL, int WIN, int G, int O>
__global__ __launch_bounds__(kBlock) void forward_mix_kernel(ForwardArgs<FD> a, MixArgs<FD> g)
{
  constexpr int H = win_halo<WIN>::value;                 // halo bins per side
  constexpr int HL = (H + BPL - 1) / BPL;                 // halo lanes per side
  constexpr int KB = cov_burst<G>::value;

  const int lane = threadIdx.x & (kWave - 1);
  const unsigned wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long wave = (unsigned long long)blockIdx.x * kWavesPerBlock + wib;
  if (wave >= a.total_waves) return;

  const unsigned tile = (unsigned)(wave % a.tiles);
  const unsigned long long rest = wave / a.tiles;
  const unsigned chunk = a.chunk0 + (unsigned)(rest % a.launch_chunks);
  const size_t item = (size_t)(rest / a.launch_chunks);
  if (item >= g.nitems) return;
  const SDFT_CONSTANT MixItem* its = as_uniform(g.items);
  const SDFT_CONSTANT unsigned* chan = as_uniform(g.chan);
  const unsigned o0 = its[item].o0, no = its[item].no;
  const bool block = no != 0, writes = its[item].writes != 0;

  const long nbins = (long)a.nbins;
  const unsigned span = 2u * a.nbins, maxc = span - 1u;
  const size_t t0 = chunk ? (size_t)chunk * a.chunk_len - a.chunk_shift : 0;
  const size_t tn = (size_t)(chunk + 1) * a.chunk_len - a.chunk_shift;
  const size_t t1 = tn < a.n ? tn : a.n;
  const unsigned c0 = (unsigned)(((size_t)a.cursor0 + t0) % span);

  // lane -> bins
  const long kfirst = (long)tile * a.interior_lanes * BPL + (long)(lane - HL) * BPL;
  const bool owner = (lane >= HL) && (lane < HL + (int)a.interior_lanes);
  // tile -> band (logic::power_tile_emits): the tile's owned bins [own0, own1) against [bin0, bin0 + nbins_out)
  const long own0 = (long)tile * a.interior_lanes * BPL;
  const long own1 = own0 + (long)a.interior_lanes * BPL < nbins ? own0 + (long)a.interior_lanes * BPL : nbins;
  const long band0 = (long)g.bin0, band1 = band0 + (long)g.nbins_out;
  const bool emits = block && own0 < band1 && band0 < own1;
  if (!emits && !writes) return;

  bool flip[BPL], live[BPL], own[BPL], keep[BPL];
  long kks[BPL];
  cx<FD> tw[BPL];
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    kks[b] = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
    keep[b] = own[b] && k >= band0 && k < band1;
    tw[b] = a.tw[kks[b]];
  }
  const bool last_chunk = (chunk + 1 == a.chunks);
  // the carry-in of the chunk for one plan channel, and the channel's state from the last chunk
  auto load = [&](BinState<FD> (&s)[BPL], size_t ch) __attribute__((always_inline))
  {
    const size_t cbase = (ch * a.chunks + chunk) * a.nbins;
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      s[b].tw = tw[b];
      s[b].acc = a.carry[cbase + kks[b]];
      s[b].fid = a.fseed ? fid_from_table(a.fseed, a.fseed_L, a.nbins, kks[b], c0, tw[b])
               : a.seed  ? a.seed[cbase + kks[b]] : a.wtab[(size_t)(((unsigned long long)kks[b] * c0) % span)];
    }
  };
  auto store = [&](const BinState<FD> (&s)[BPL], size_t ch) __attribute__((always_inline))
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (own[b])
      {
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
  };

  if (!emits)
  {
    // no row to form: the channels this item writes, one after the other, acc and fid only
    const unsigned nadv = block ? g.nch : 1u;
    for (unsigned q = 0; q < nadv; ++q)
    {
      const size_t ch = block ? chan[q] : o0;
      BinState<FD> s[BPL];
      load(s, ch);
      const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
      unsigned c = c0;
      size_t t = t0;
      while (t < t1)
      {
        size_t run = maxc - c;                             // normal steps before the roll-over
        if (run > t1 - t) run = t1 - t;
        const size_t end = t + run;
        for (; t + kGroup <= end; t += kGroup)
        {
          FD dl[kGroup];
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
          for (int u = 0; u < kGroup; ++u)
          {
#pragma unroll
            for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl[u]);
          }
        }
        for (; t < end; ++t)
        {
          const FD dl = d[t];
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl);
        }
        c += (unsigned)run;
        if (t < t1)
        {
          const FD dl = d[t];
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_wrap(s[b], dl);
          ++t; c = 0;
        }
      }
      if (last_chunk) store(s, ch);
    }
    return;
  }

  // ---- a block that forms rows ----
  const unsigned top = g.nch - 1u;
  const FD w = a.wscale;
  const size_t nb2 = 2 * (size_t)g.nbins_out;              // FD numbers per row

  // the chunk's first grid sample and its row (wave-uniform; one division per wave)
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  size_t next0 = first;
  if (t0 > first) next0 = first + ((t0 - first + every - 1) / every) * every;
  // this lane's first bin in that row of the block's first output
  FD* const dst0 = g.out + (size_t)o0 * g.out_stride + ((next0 - first) / every) * nb2 + 2 * (kfirst - band0);

  // the windowed bins of one channel from its demodulated bins
  auto taps = [&](cx<FD> (&x)[BPL], cx<FD> (&y)[BPL]) __attribute__((always_inline))
  {
    // mirror lanes conjugate; N == 1 halo is zero
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      if (flip[b]) x[b].im = -x[b].im;
      if (!live[b]) x[b] = cmake<FD>((FD)0, (FD)0);
    }
    // gather X[k-2..k+2] for every bin of the lane
    cx<FD> e[BPL + 4] = {};
#pragma unroll
    for (int b = 0; b < BPL; ++b) e[b + 2] = x[b];
    if constexpr (H >= 1)
    {
      e[1] = from_below(x[BPL - 1]);
      e[BPL + 2] = from_above(x[0]);
    }
    if constexpr (H >= 2)
    {
      if constexpr (BPL >= 2)
      {
        e[0] = from_below(x[BPL - 2]);
        e[BPL + 3] = from_above(x[1]);
      }
      else
      {
        e[0] = from_below(e[1]);
        e[BPL + 3] = from_above(e[BPL + 2]);
      }
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b) y[b] = window_tap<FD, WIN>(e[b], e[b + 1], e[b + 2], e[b + 3], e[b + 4], w);
  };
  // A lane holds 16 bytes of a row (one double pair, two float pairs); the row is aligned to sizeof(FD) only.  The running sum
  // comes back in the form it was stored in: the tests on keep and on the address are the same in both directions.
  auto load_sum = [&](const FD* p, FD (&re)[BPL], FD (&im)[BPL]) __attribute__((always_inline))
  {
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(p) & 15u) == 0)
      {
        using V = typename StoreVec<FD, 2>::type;
        const V v = *reinterpret_cast<const V*>(p);
        re[0] = v.x; im[0] = v.y; re[1] = v.z; im[1] = v.w;
        return;
      }
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      re[b] = (FD)-0.0; im[b] = (FD)-0.0;
      if (!keep[b]) continue;
      const FD* q = p + 2 * b;
      if ((reinterpret_cast<size_t>(q) & (2 * sizeof(FD) - 1)) == 0)
      {
        using V = typename StoreVec<FD, 1>::type;
        const V v = *reinterpret_cast<const V*>(q);
        re[b] = v.x; im[b] = v.y;
      }
      else { re[b] = q[0]; im[b] = q[1]; }
    }
  };
  auto store_sum = [&](FD* p, const FD (&re)[BPL], const FD (&im)[BPL]) __attribute__((always_inline))
  {
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(p) & 15u) == 0)
      {
        using V = typename StoreVec<FD, 2>::type;
        V v; v.x = re[0]; v.y = im[0]; v.z = re[1]; v.w = im[1];
        store_vec(reinterpret_cast<V*>(p), v);
        return;
      }
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      if (!keep[b]) continue;
      FD* q = p + 2 * b;
      if ((reinterpret_cast<size_t>(q) & (2 * sizeof(FD) - 1)) == 0)
      {
        using V = typename StoreVec<FD, 1>::type;
        V v; v.x = re[b]; v.y = im[b];
        store_vec(reinterpret_cast<V*>(q), v);
      }
      else { q[0] = re[b]; q[1] = im[b]; }
    }
  };

  for (unsigned e0 = 0; e0 < g.nch; e0 += G)
  {
    const unsigned ng = g.nch - e0 < (unsigned)G ? g.nch - e0 : (unsigned)G;      // elements of the group (wave-uniform)
    const bool opens = e0 == 0;                            // the first group starts the sums
    size_t chs[G];
    BinState<FD> s[G][BPL];
    const SDFT_CONSTANT FD* d[G];
    FD wr[O][G][BPL], wi[O][G][BPL];
#pragma unroll
    for (int i = 0; i < G; ++i)
    {
      const unsigned el = e0 + i < top ? e0 + i : top;     // (a padded slot: the mix's last channel once more)
      chs[i] = chan[el];
      load(s[i], chs[i]);
      d[i] = as_uniform(a.delta + chs[i] * a.n);
#pragma unroll
      for (int o = 0; o < O; ++o)
      {
        const unsigned oo = (unsigned)o < no ? o0 + o : o0;
        const cx<FD>* wrow = g.weights + ((size_t)oo * g.nch + el) * a.nbins;
#pragma unroll
        for (int b = 0; b < BPL; ++b)
        {
          wr[o][i][b] = (FD)0; wi[o][i][b] = (FD)0;
          if (keep[b]) { const cx<FD> v = wrow[kfirst + b]; wr[o][i][b] = v.re; wi[o][i][b] = v.im; }
        }
      }
    }

    size_t next = next0;
    FD* dst = dst0;
    // one grid sample: the G recurrences step, each channel is windowed once, and every output of the block continues its sum
    auto sample = [&](const FD (&dl)[G], const bool wrap) __attribute__((always_inline))
    {
      cx<FD> y[G][BPL];
#pragma unroll
      for (int i = 0; i < G; ++i)
      {
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = wrap ? step_wrap(s[i][b], dl[i]) : step_normal(s[i][b], dl[i]);
        taps(x, y[i]);
      }
#pragma unroll
      for (int o = 0; o < O; ++o)
      {
        if ((unsigned)o >= no) continue;                   // wave-uniform
        FD* const p = dst + (size_t)o * g.out_stride;
        FD re[BPL], im[BPL];
        if (opens)
        {
#pragma unroll
          for (int b = 0; b < BPL; ++b) { re[b] = (FD)-0.0; im[b] = (FD)-0.0; }
        }
        else load_sum(p, re, im);
#pragma unroll
        for (int i = 0; i < G; ++i)
        {
          if ((unsigned)i >= ng) continue;                 // wave-uniform: a padded slot adds nothing
#pragma unroll
          for (int b = 0; b < BPL; ++b)
          {
            const FD rr = wr[o][i][b] * y[i][b].re, ii = wi[o][i][b] * y[i][b].im;
            const FD ri = wr[o][i][b] * y[i][b].im, ir = wi[o][i][b] * y[i][b].re;
            const FD tre = rr - ii, tim = ri + ir;
            re[b] = re[b] + tre;
            im[b] = im[b] + tim;
          }
        }
        store_sum(p, re, im);
      }
      dst += nb2; next += every;
    };
    auto one = [&](size_t t, const bool wrap, const bool row) __attribute__((always_inline))
    {
      FD dl[G];
#pragma unroll
      for (int i = 0; i < G; ++i) dl[i] = d[i][t];
      if (row) { sample(dl, wrap); return; }
#pragma unroll
      for (int i = 0; i < G; ++i)
      {
#pragma unroll
        for (int b = 0; b < BPL; ++b) { if (wrap) advance_wrap(s[i][b], dl[i]); else advance_normal(s[i][b], dl[i]); }
      }
    };

    unsigned c = c0;
    size_t t = t0;
    while (t < t1)
    {
      size_t run = maxc - c;                               // normal steps before the roll-over
      if (run > t1 - t) run = t1 - t;
      const size_t end = t + run;
      while (t < end)
      {
        if (t == next)
        {
          if (every == 1 && t + KB <= end)
          {
            // the dense grid: one s_load burst per channel and KB samples, each of them a row
            FD dl[KB][G];
#pragma unroll
            for (int i = 0; i < G; ++i)
#pragma unroll
              for (int u = 0; u < KB; ++u) dl[u][i] = d[i][t + u];
#pragma unroll
            for (int u = 0; u < KB; ++u) sample(dl[u], false);
            t += KB;
            continue;
          }
          one(t, false, true);
          ++t;
          continue;
        }
        const size_t stop = next < end ? next : end;       // samples whose rows nobody keeps: acc and fid only
        for (; t + KB <= stop; t += KB)
        {
          FD dl[KB][G];
#pragma unroll
          for (int i = 0; i < G; ++i)
#pragma unroll
            for (int u = 0; u < KB; ++u) dl[u][i] = d[i][t + u];
#pragma unroll
          for (int u = 0; u < KB; ++u)
#pragma unroll
            for (int i = 0; i < G; ++i)
#pragma unroll
              for (int b = 0; b < BPL; ++b) advance_normal(s[i][b], dl[u][i]);
        }
        for (; t < stop; ++t) one(t, false, false);
      }
      c += (unsigned)run;
      if (t < t1)
      {
        one(t, true, t == next);
        ++t; c = 0;
      }
    }

    if (last_chunk && writes)
    {
#pragma unroll
      for (int i = 0; i < G; ++i)
        if ((unsigned)i < ng) store(s[i], chs[i]);
    }
  }
}

}  // namespace sdfthip
