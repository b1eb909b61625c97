// sdft_forward_cross_sum.hpp -- K1x: pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n), A conj(B) of the windowed bins of
// two channels of a plan summed over the windows of a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_power_sum.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// One work item of a cross-spectrum call (logic::cross_items): the channels whose recurrences the wave steps, the pair whose sums
// it forms (out < 0: none, the item only advances channel a) and which sides write their channel's state back on the last chunk
// (over all items every channel has exactly one writer).
struct CrossItem
{
  unsigned a, b;
  int out;
  unsigned short writes_a, writes_b;
};

// Windows, rows and head row as PowerSumArgs; every element is a complex number stored as (re, im), so in FD units a row is
// 2 * nbins_out long: bin k of row 0 of pair p goes to row0 + p * row0_stride + 2 * (k - bin0), of row r >= 1 to
// rest + p * rest_stride + (r - 1) * 2 * nbins_out + 2 * (k - bin0) (strides in FD units).  ws is the workspace of the windows a
// chunk boundary cuts, [items][chunks][2][nbins_out] complex; the items of the pairs come first and in the pairs' order, so item i
// is pair i there and pooled_power_rows_kernel adds the pieces as real sums over 2 * nbins_out numbers of `npairs` channels.
template <typename FD> struct CrossSumArgs
{
  FD* row0;                   // [npairs][nbins_out] complex, aligned to sizeof(FD) only
  size_t row0_stride;
  FD* rest;                   // [npairs][rows - 1][nbins_out] complex, likewise
  size_t rest_stride;
  FD* ws;                     // nullptr for a call of one chunk
  const CrossItem* items;     // [nitems]
  unsigned nitems, npairs;
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// forward_pooled_power_kernel with a second channel.  A wave is (tile, chunk, item); it takes the carry-in of the chunk for the
// channels a and b of its item (the carries of all channels are complete before this kernel starts: grid calls never run in flow
// mode), steps both recurrences sample by sample, windows both from their own halo lanes and forms, with A and B the windowed
// bins and no fused multiply-add,
//   re = fl(fl(A.re * B.re) + fl(A.im * B.im))        im = fl(fl(A.im * B.re) - fl(A.re * B.im))
// which it adds to two accumulators per bin, in time order, in FD.  An item with a == b steps one recurrence and uses its bin
// for both sides (the same operations on the same numbers: the same bits); re is then the pooled power call's term and im is
// x - x = +0.  Windows, flushes, workspace slots and bursts are forward_pooled_power_kernel's.  Tiles outside the band and items
// without a pair only step the recurrences.  On the last chunk a side marked as writer stores its channel's state.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_cross_sum_kernel(ForwardArgs<FD> a, CrossSumArgs<FD> g)
{
  constexpr int H = win_halo<WIN>::value;                 // halo bins per side
  constexpr int HL = (H + BPL - 1) / BPL;                 // halo lanes per side

  const int lane = threadIdx.x & (kWave - 1);
  const unsigned wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long wave = (unsigned long long)blockIdx.x * kWavesPerBlock + wib;
  if (wave >= a.total_waves) return;

  const unsigned tile = (unsigned)(wave % a.tiles);
  const unsigned long long rest = wave / a.tiles;
  const unsigned chunk = a.chunk0 + (unsigned)(rest % a.launch_chunks);
  const size_t item = (size_t)(rest / a.launch_chunks);
  if (item >= g.nitems) return;
  const SDFT_CONSTANT CrossItem* its = as_uniform(g.items);
  const size_t cha = its[item].a, chb = its[item].b;
  const int pair = its[item].out;
  const bool writes_a = its[item].writes_a != 0, writes_b = its[item].writes_b != 0;
  const bool dual = cha != chb;                            // wave-uniform

  const long nbins = (long)a.nbins;
  const unsigned span = 2u * a.nbins, maxc = span - 1u;
  const size_t t0 = chunk ? (size_t)chunk * a.chunk_len - a.chunk_shift : 0;
  const size_t tn = (size_t)(chunk + 1) * a.chunk_len - a.chunk_shift;
  const size_t t1 = tn < a.n ? tn : a.n;
  unsigned c = (unsigned)(((size_t)a.cursor0 + t0) % span);

  // lane -> bins
  const long kfirst = (long)tile * a.interior_lanes * BPL + (long)(lane - HL) * BPL;
  const bool owner = (lane >= HL) && (lane < HL + (int)a.interior_lanes);
  // tile -> band (logic::power_tile_emits): the tile's owned bins [own0, own1) against [bin0, bin0 + nbins_out)
  const long own0 = (long)tile * a.interior_lanes * BPL;
  const long own1 = own0 + (long)a.interior_lanes * BPL < nbins ? own0 + (long)a.interior_lanes * BPL : nbins;
  const long band0 = (long)g.bin0, band1 = band0 + (long)g.nbins_out;
  const bool emits = pair >= 0 && own0 < band1 && band0 < own1;

  BinState<FD> sa[BPL], sb[BPL];
  bool flip[BPL], live[BPL], own[BPL], keep[BPL];
  const size_t cbase_a = (cha * a.chunks + chunk) * a.nbins, cbase_b = (chb * a.chunks + chunk) * a.nbins;
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    const long kk = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
    keep[b] = own[b] && k >= band0 && k < band1;
    sa[b].tw = a.tw[kk];
    sa[b].acc = a.carry[cbase_a + kk];
    sa[b].fid = a.fseed ? fid_from_table(a.fseed, a.fseed_L, a.nbins, kk, c, sa[b].tw)
              : a.seed  ? a.seed[cbase_a + kk] : a.wtab[(size_t)(((unsigned long long)kk * c) % span)];
    sb[b] = sa[b];
    if (dual)
    {
      sb[b].acc = a.carry[cbase_b + kk];
      if (!a.fseed && a.seed) sb[b].fid = a.seed[cbase_b + kk];
    }
  }

  const SDFT_CONSTANT FD* da = as_uniform(a.delta + cha * a.n);
  const SDFT_CONSTANT FD* db = as_uniform(a.delta + chb * a.n);
  const FD w = a.wscale;
  const bool last_chunk = (chunk + 1 == a.chunks);
  const size_t nb2 = 2 * (size_t)g.nbins_out;              // FD numbers per row

  // the window the chunk starts in (wave-uniform; one division per wave): its row, whether it began before the chunk, and `next`,
  // the grid point that ends it
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  size_t row = 0, next = first;
  bool cut = t0 > 0;                                       // the window began before the chunk
  if (t0 >= first)
  {
    const size_t j = (t0 - first) / every;
    row = (first > 0 ? 1 : 0) + j;
    next = first + (j + 1) * every;
    cut = first + j * every < t0;
  }
  // (an empty accumulator is -0: -0 + x is x for every x, a zero of either sign included, so a window of one sample is its term
  // bit for bit; every flush follows at least one sample)
  FD sre[BPL], sim[BPL];
#pragma unroll
  for (int b = 0; b < BPL; ++b) { sre[b] = (FD)-0.0; sim[b] = (FD)-0.0; }

  // the window's samples of this chunk end at sample t (exclusive): a whole row, or a piece for the workspace.  A lane holds
  // 16 bytes of a row (one double pair, two float pairs); the row is aligned to sizeof(FD) only
  auto flush = [&](size_t t) __attribute__((always_inline))
  {
    const size_t wend = next < a.n ? next : a.n;
    const size_t p = (size_t)pair;
    FD* dst;
    if (!cut && t == wend) dst = row ? g.rest + p * g.rest_stride + (row - 1) * nb2 : g.row0 + p * g.row0_stride;
    else dst = g.ws + ((p * a.chunks + chunk) * 2 + (cut ? 0 : 1)) * nb2;
    dst += 2 * (kfirst - band0);
    bool done = false;
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 15u) == 0)
      {
        using V = typename StoreVec<FD, 2>::type;
        V v; v.x = sre[0]; v.y = sim[0]; v.z = sre[1]; v.w = sim[1];
        store_vec(reinterpret_cast<V*>(dst), v);
        done = true;
      }
    }
    if (!done)
    {
#pragma unroll
      for (int b = 0; b < BPL; ++b)
      {
        if (!keep[b]) continue;
        FD* q = dst + 2 * b;
        if ((reinterpret_cast<size_t>(q) & (2 * sizeof(FD) - 1)) == 0)
        {
          using V = typename StoreVec<FD, 1>::type;
          V v; v.x = sre[b]; v.y = sim[b];
          store_vec(reinterpret_cast<V*>(q), v);
        }
        else { q[0] = sre[b]; q[1] = sim[b]; }
      }
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b) { sre[b] = (FD)-0.0; sim[b] = (FD)-0.0; }
    ++row; next += every; cut = false;
  };

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
  auto add = [&](const cx<FD> (&ya)[BPL], const cx<FD> (&yb)[BPL]) __attribute__((always_inline))
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      const FD rr = ya[b].re * yb[b].re, ii = ya[b].im * yb[b].im;
      const FD ir = ya[b].im * yb[b].re, ri = ya[b].re * yb[b].im;
      const FD re = rr + ii, im = ir - ri;
      sre[b] = sre[b] + re;
      sim[b] = sim[b] + im;
    }
  };
  // one sample of the window: both recurrences, both windows, the term
  auto pool_normal = [&](FD dla, FD dlb) __attribute__((always_inline))
  {
    cx<FD> xa[BPL], ya[BPL];
#pragma unroll
    for (int b = 0; b < BPL; ++b) xa[b] = step_normal(sa[b], dla);
    taps(xa, ya);
    if (dual)
    {
      cx<FD> xb[BPL], yb[BPL];
#pragma unroll
      for (int b = 0; b < BPL; ++b) xb[b] = step_normal(sb[b], dlb);
      taps(xb, yb);
      add(ya, yb);
    }
    else add(ya, ya);
  };
  auto pool_wrap = [&](FD dla, FD dlb) __attribute__((always_inline))
  {
    cx<FD> xa[BPL], ya[BPL];
#pragma unroll
    for (int b = 0; b < BPL; ++b) xa[b] = step_wrap(sa[b], dla);
    taps(xa, ya);
    if (dual)
    {
      cx<FD> xb[BPL], yb[BPL];
#pragma unroll
      for (int b = 0; b < BPL; ++b) xb[b] = step_wrap(sb[b], dlb);
      taps(xb, yb);
      add(ya, yb);
    }
    else add(ya, ya);
  };

  size_t t = t0;
  while (t < t1)
  {
    size_t run = maxc - c;                                 // normal steps before the roll-over
    if (run > t1 - t) run = t1 - t;
    const size_t end = t + run;
    if (emits)
    {
      while (t < end)
      {
        if (t == next) flush(t);
        const size_t stop = next < end ? next : end;       // the window's samples before the roll-over
        for (; t + kGroup <= stop; t += kGroup)            // one s_load burst per channel and kGroup samples
        {
          FD dla[kGroup], dlb[kGroup];
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dla[u] = da[t + u];
          if (dual)                                          // (one channel: one stream of differences)
          {
#pragma unroll
            for (int u = 0; u < kGroup; ++u) dlb[u] = db[t + u];
          }
          else
          {
#pragma unroll
            for (int u = 0; u < kGroup; ++u) dlb[u] = dla[u];
          }
#pragma unroll
          for (int u = 0; u < kGroup; ++u) pool_normal(dla[u], dlb[u]);
        }
        for (; t < stop; ++t) { const FD dla = da[t]; pool_normal(dla, dual ? db[t] : dla); }
      }
    }
    else
    {
      for (; t + kGroup <= end; t += kGroup)               // no bin to sum: acc and fid only
      {
        FD dla[kGroup], dlb[kGroup];
#pragma unroll
        for (int u = 0; u < kGroup; ++u) dla[u] = da[t + u];
        if (dual)
        {
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dlb[u] = db[t + u];
        }
        else
        {
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dlb[u] = dla[u];
        }
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
        {
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(sa[b], dla[u]);
          if (dual)
          {
#pragma unroll
            for (int b = 0; b < BPL; ++b) advance_normal(sb[b], dlb[u]);
          }
        }
      }
      for (; t < end; ++t)
      {
        const FD dla = da[t], dlb = dual ? db[t] : dla;
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_normal(sa[b], dla);
        if (dual)
        {
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(sb[b], dlb);
        }
      }
    }
    c += (unsigned)run;
    if (t < t1)
    {
      const FD dla = da[t], dlb = dual ? db[t] : dla;
      if (emits)
      {
        if (t == next) flush(t);
        pool_wrap(dla, dlb);
      }
      else
      {
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_wrap(sa[b], dla);
        if (dual)
        {
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_wrap(sb[b], dlb);
        }
      }
      ++t; c = 0;
    }
  }
  if (emits) flush(t1);                                    // (t1 > t0: the last window of the chunk has samples)

  if (last_chunk)
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (own[b])
      {
        if (writes_a)
        {
          a.acc_state[cha * a.nbins + kfirst + b] = sa[b].acc;
          a.fid_state[cha * a.nbins + kfirst + b] = sa[b].fid;
        }
        if (dual && writes_b)
        {
          a.acc_state[chb * a.nbins + kfirst + b] = sb[b].acc;
          a.fid_state[chb * a.nbins + kfirst + b] = sb[b].fid;
        }
      }
  }
}

}  // namespace sdfthip
