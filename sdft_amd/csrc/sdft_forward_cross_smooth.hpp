// sdft_forward_cross_smooth.hpp -- K1xs: smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n), the one-pole average
// s[t] = fl(fl(a * s[t - 1]) + fl(b * A conj(B))) per component of the windowed bins of two channels of a plan, kept on a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_cross_sum.hpp"
#include "sdft_forward_power_smooth.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// Every element is a complex number stored as (re, im), so in FD units a row is 2 * nbins_out long: bin k of the row of grid point
// first + r * every of pair p goes to out + p * out_stride + r * 2 * nbins_out + 2 * (k - bin0) (out_stride in FD units).
// state_in / state_out: [npairs][nbins_out] complex, s before the call's first sample and after its last, as PowerSmoothArgs' --
// two buffers; state_out is written by the forward kernel in a call of one chunk (ends == nullptr), by smooth_scan_kernel otherwise.
// ends: the workspace [npairs][chunks][nbins_out] complex of a call of more than one chunk.  The items of the pairs come first and
// in the pairs' order, so item i is pair i there and smooth_scan_kernel / smooth_fix_kernel carry the pieces as real numbers:
// 2 * nbins_out per row of `npairs` channels.
template <typename FD> struct CrossSmoothArgs
{
  FD* out;                    // [npairs][rows][nbins_out] complex, aligned to sizeof(FD) only; nullptr: the call keeps no row
  size_t out_stride;          // FD numbers per pair
  const FD* state_in;         // never nullptr (the plan's buffers)
  FD* state_out;
  FD* ends;                   // nullptr for a call of one chunk
  const CrossItem* items;     // [nitems]
  unsigned nitems, npairs;
  FD a, b;                    // the rounded decay and fl(1 - a)
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// forward_cross_sum_kernel (the (tile, chunk, item) wave, the dual and the single recurrence, halo, taps, the term, emits, the
// writers of the channel states) with forward_power_smooth_kernel's recursion for the sums: the term (re, im) of EVERY sample
// enters two accumulators per bin as s = fl(fl(a * s) + fl(b * term)), each component on its own, no fused multiply-add.  At a grid
// point the accumulators are stored AFTER that sample's step and are not cleared.  Chunk 0 starts from the incoming state, every
// later chunk from +0; the end values go to the workspace, or -- a call of one chunk -- to the state.  An item with a == b forms
// re exactly as forward_power_smooth_kernel forms its term and im = x - x = +0, which keeps a +0 accumulator at +0.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_cross_smooth_kernel(ForwardArgs<FD> a, CrossSmoothArgs<FD> g)
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
  const size_t nb2 = 2 * (size_t)g.nbins_out;              // FD numbers per row
  const size_t unit = emits ? (size_t)pair : 0;

  BinState<FD> sa[BPL], sb[BPL];
  bool flip[BPL], live[BPL], own[BPL], keep[BPL];
  const size_t cbase_a = (cha * a.chunks + chunk) * a.nbins, cbase_b = (chb * a.chunks + chunk) * a.nbins;
  FD sre[BPL], sim[BPL];                                   // the smoothed cross-spectrum of the lane's bins
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    const long kk = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
    keep[b] = emits && own[b] && k >= band0 && k < band1;
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
    sre[b] = (FD)0; sim[b] = (FD)0;
    if (chunk == 0 && keep[b])
    {
      const FD* const sp = g.state_in + unit * nb2 + 2 * (size_t)(k - band0);
      sre[b] = sp[0]; sim[b] = sp[1];
    }
  }

  const SDFT_CONSTANT FD* da = as_uniform(a.delta + cha * a.n);
  const SDFT_CONSTANT FD* db = as_uniform(a.delta + chb * a.n);
  const FD w = a.wscale;
  const FD ca = g.a, cb = g.b;
  const bool last_chunk = (chunk + 1 == a.chunks);

  // the first grid point at or after t0 (wave-uniform; one division per wave): its row, and `next`, the sample after it -- the
  // row is stored on the way into sample `next`, or at the chunk's end.  A grid without a point in the call never stores.
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  size_t row = 0, next = first < a.n ? first + 1 : ~(size_t)0;
  if (t0 > first)
  {
    row = (t0 - first + every - 1) / every;
    next = first + row * every + 1;
  }

  // 16 bytes of a row per lane (one double pair, two float pairs); the row is aligned to sizeof(FD) only
  auto put = [&](FD* dst) __attribute__((always_inline))
  {
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
  };
  // the grid point t - 1 has been stepped: its row goes out, the accumulators stay
  auto store_row = [&]() __attribute__((always_inline))
  {
    put(g.out + unit * g.out_stride + row * nb2 + 2 * (kfirst - band0));
    ++row; next += every;
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
  auto smooth = [&](const cx<FD> (&ya)[BPL], const cx<FD> (&yb)[BPL]) __attribute__((always_inline))
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      const FD rr = ya[b].re * yb[b].re, ii = ya[b].im * yb[b].im;
      const FD ir = ya[b].im * yb[b].re, ri = ya[b].re * yb[b].im;
      const FD re = rr + ii, im = ir - ri;
      const FD asr = ca * sre[b], bre = cb * re;
      const FD asi = ca * sim[b], bim = cb * im;
      sre[b] = asr + bre;
      sim[b] = asi + bim;
    }
  };
  // one sample: both recurrences, both windows, the term, the recursion
  auto step_n = [&](FD dla, FD dlb) __attribute__((always_inline))
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
      smooth(ya, yb);
    }
    else smooth(ya, ya);
  };
  auto step_w = [&](FD dla, FD dlb) __attribute__((always_inline))
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
      smooth(ya, yb);
    }
    else smooth(ya, ya);
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
        if (t == next) store_row();
        const size_t stop = next < end ? next : end;       // the samples up to the next grid point, before the roll-over
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
          for (int u = 0; u < kGroup; ++u) step_n(dla[u], dlb[u]);
        }
        for (; t < stop; ++t) { const FD dla = da[t]; step_n(dla, dual ? db[t] : dla); }
      }
    }
    else
    {
      for (; t + kGroup <= end; t += kGroup)               // no bin to smooth: acc and fid only
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
        if (t == next) store_row();
        step_w(dla, dlb);
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
  if (emits)
  {
    if (t1 == next) store_row();                           // the chunk's last sample is a grid point
    // what the chunk ends with: E_c for the scan, or -- a call of one chunk -- the state itself
    FD* const endp = g.ends ? g.ends + (unit * a.chunks + chunk) * nb2 : g.state_out + unit * nb2;
    put(endp + 2 * (kfirst - band0));
  }

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
