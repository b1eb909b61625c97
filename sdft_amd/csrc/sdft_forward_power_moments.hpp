// sdft_forward_power_moments.hpp -- K1q: power-moments analysis (sdft_hip_sdft_power_moments_n), |X|^2 and its square of a band of
// bins, each summed over the windows of a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_cross_sum.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// forward_pooled_power_kernel with a second accumulator per bin: its geometry, carry-in, halo, window taps, band test, bursts of
// kGroup, roll-over step, flush rule and state write-back, line for line.  The term of a sample is the pooled call's
//   p = fl(fl(re * re) + fl(im * im))
// of the windowed bin, then q = fl(p * p) (no fused multiply-add), then s1 = s1 + p and s2 = s2 + q: s1 sees the operations of the
// pooled kernel's one accumulator in the same order from the same +0 start, which is why [..][0] has that call's bits.  q overflows
// to inf in IEEE fashion; nothing is done about it.
// The output interleaves the two sums, (s1, s2) per bin, so a row of nbins_out pairs is the cross-spectrum call's row of nbins_out
// complex numbers: the arguments are that call's CrossSumArgs with the plan's channels in the pairs' place (items is unused,
// nitems == npairs == channels), as the lag-product call has them.  The workspace of the windows a chunk boundary cuts is
// [channels][chunks][2][nbins_out] pairs, and pooled_power_rows_kernel adds the pieces as real sums over 2 * nbins_out numbers --
// each component in the order the pooled call adds its own.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_power_moments_kernel(ForwardArgs<FD> a, CrossSumArgs<FD> g)
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
  const size_t ch = (size_t)(rest / a.launch_chunks);
  if (ch >= g.npairs) return;

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
  const bool emits = own0 < band1 && band0 < own1;

  BinState<FD> s[BPL];
  bool flip[BPL], live[BPL], own[BPL], keep[BPL];
  const size_t cbase = (ch * a.chunks + chunk) * a.nbins;
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    const long kk = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
    keep[b] = own[b] && k >= band0 && k < band1;
    s[b].tw = a.tw[kk];
    s[b].acc = a.carry[cbase + kk];
    s[b].fid = a.fseed ? fid_from_table(a.fseed, a.fseed_L, a.nbins, kk, c, s[b].tw)
             : a.seed  ? a.seed[cbase + kk] : a.wtab[(size_t)(((unsigned long long)kk * c) % span)];
  }

  const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
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
  // (both accumulators start where the pooled kernel's one does: +0)
  FD s1[BPL], s2[BPL];
#pragma unroll
  for (int b = 0; b < BPL; ++b) { s1[b] = (FD)0; s2[b] = (FD)0; }

  // the window's samples of this chunk end at sample t (exclusive): a whole row, or a piece for the workspace.  A lane's pairs
  // are adjacent in the row (one double pair, two float pairs: 16 bytes); the row is aligned to sizeof(FD) only and the band's
  // edges cut lanes, so every vector store has its scalar fallback
  auto flush = [&](size_t t) __attribute__((always_inline))
  {
    const size_t wend = next < a.n ? next : a.n;
    FD* dst;
    if (!cut && t == wend) dst = row ? g.rest + ch * g.rest_stride + (row - 1) * nb2 : g.row0 + ch * g.row0_stride;
    else dst = g.ws + ((ch * a.chunks + chunk) * 2 + (cut ? 0 : 1)) * nb2;
    dst += 2 * (kfirst - band0);
    bool done = false;
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 15u) == 0)
      {
        using V = typename StoreVec<FD, 2>::type;
        V v; v.x = s1[0]; v.y = s2[0]; v.z = s1[1]; v.w = s2[1];
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
          V v; v.x = s1[b]; v.y = s2[b];
          store_vec(reinterpret_cast<V*>(q), v);
        }
        else { q[0] = s1[b]; q[1] = s2[b]; }
      }
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b) { s1[b] = (FD)0; s2[b] = (FD)0; }
    ++row; next += every; cut = false;
  };

  auto pool = [&](cx<FD> (&x)[BPL]) __attribute__((always_inline))
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
    for (int b = 0; b < BPL; ++b)
    {
      const cx<FD> y = window_tap<FD, WIN>(e[b], e[b + 1], e[b + 2], e[b + 3], e[b + 4], w);
      const FD rr = y.re * y.re, ii = y.im * y.im;
      const FD p = rr + ii;
      const FD q = p * p;
      s1[b] = s1[b] + p;
      s2[b] = s2[b] + q;
    }
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
        for (; t + kGroup <= stop; t += kGroup)            // one s_load burst per kGroup samples
        {
          FD dl[kGroup];
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
          for (int u = 0; u < kGroup; ++u)
          {
            cx<FD> x[BPL];
#pragma unroll
            for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl[u]);
            pool(x);
          }
        }
        for (; t < stop; ++t)
        {
          const FD dl = d[t];
          cx<FD> x[BPL];
#pragma unroll
          for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl);
          pool(x);
        }
      }
    }
    else
    {
      for (; t + kGroup <= end; t += kGroup)               // no bin of the band: acc and fid only
      {
        FD dl[kGroup];
#pragma unroll
        for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl[u]);
      }
      for (; t < end; ++t)
      {
        const FD dl = d[t];
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl);
      }
    }
    c += (unsigned)run;
    if (t < t1)
    {
      const FD dl = d[t];
      if (emits)
      {
        if (t == next) flush(t);
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = step_wrap(s[b], dl);
        pool(x);
      }
      else
      {
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_wrap(s[b], dl);
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
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
  }
}

}  // namespace sdfthip
