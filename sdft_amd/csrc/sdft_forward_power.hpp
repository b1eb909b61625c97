// sdft_forward_power.hpp -- K1p: power-spectrogram analysis (sdft_hip_sdft_power_n), |X|^2 of a band of bins on a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp); citations are into /root/reference/c/src/sdft/sdft.h.

#pragma once

#include "sdft_forward_every.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// the call-local row grid of EveryGrid plus a band of bins: bin k of row r of channel ch, bin0 <= k < bin0 + nbins_out, goes
// to out + ch * out_stride + r * nbins_out + (k - bin0) as one real number
template <typename FD> struct PowerArgs
{
  FD* out;                    // [channels][rows][nbins_out], aligned to sizeof(FD) only
  size_t out_stride;          // elements per channel
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// forward_every_kernel's geometry, carry-in and time loop; the windowed bin never leaves the registers as a complex number:
// fl(fl(re * re) + fl(im * im)) is formed in FD (no fused multiply-add: the expression numpy evaluates on the reference's row)
// and stored for the band's bins only.  A tile that owns no bin of the band (a wave-uniform test) keeps no row at all: its
// `next` lies past every sample, so it runs the acc / fid loop over the whole chunk and writes the state like any other tile.
// Tiles that emit window their bins from halo lanes as ever, whether the neighbours are in the band or not.
// forward_every_kernel never sees a dense grid (every == 1 is sdft_sdft_n there); this one does, and then loads the
// differences in bursts of kGroup like forward_kernel.
// A lane holds 8 bytes of a row (one double, two floats): FD float stores them as one dwordx2 where both bins are in the band
// and the address allows it, else bin by bin (a band of an odd length changes the alignment from row to row).
// (A 16-byte form -- neighbouring lanes exchange over DPP, two consecutive kept rows leave as one dwordx4 per lane -- was built,
// measured and dropped: the kernel is bound by the arithmetic of its rows and the exchange adds to it; configs[1], every row, all
// bins 2.196 against 2.153 ms, configs[2] 2.525 against 2.351 ms, profiles/power_rates.txt.)
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_power_kernel(ForwardArgs<FD> a, PowerArgs<FD> g)
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

  // the chunk's first grid sample and its row (wave-uniform; one division per wave); a tile outside the band has none
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  size_t next = first;
  if (t0 > first) next = first + ((t0 - first + every - 1) / every) * every;
  const size_t row = emits ? (next - first) / every : 0;
  if (!emits) next = ~(size_t)0;
  FD* dst = g.out + ch * g.out_stride + row * (size_t)g.nbins_out + (kfirst - band0);

  auto emit = [&](cx<FD> (&x)[BPL]) __attribute__((always_inline))
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
    FD p[BPL];
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      const cx<FD> y = window_tap<FD, WIN>(e[b], e[b + 1], e[b + 2], e[b + 3], e[b + 4], w);
      const FD rr = y.re * y.re, ii = y.im * y.im;
      p[b] = rr + ii;
    }

    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 7u) == 0)
      {
        using V = typename StoreVec<FD, 1>::type;
        V v; v.x = p[0]; v.y = p[1];
        store_vec(reinterpret_cast<V*>(dst), v);
      }
      else
      {
        if (keep[0]) dst[0] = p[0];
        if (keep[1]) dst[1] = p[1];
      }
    }
    else
    {
      if (keep[0]) dst[0] = p[0];
    }
    dst += g.nbins_out;
  };

  size_t t = t0;
  while (t < t1)
  {
    size_t run = maxc - c;                                 // normal steps before the roll-over
    if (run > t1 - t) run = t1 - t;
    const size_t end = t + run;
    while (t < end)
    {
      if (t == next)
      {
        if (every <= (size_t)kGroup && t + kGroup <= end)
        {
          // a dense grid: one s_load burst per kGroup samples here too, each of them a row or a step
          FD dl[kGroup];
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
          for (int u = 0; u < kGroup; ++u)
          {
            if (t + u == next)
            {
              cx<FD> x[BPL];
#pragma unroll
              for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl[u]);
              emit(x);
              next += every;
            }
            else
            {
#pragma unroll
              for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl[u]);
            }
          }
          t += kGroup;
          continue;
        }
        const FD dl = d[t];
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl);
        emit(x);
        next += every;
        ++t;
        continue;
      }
      const size_t stop = next < end ? next : end;         // samples whose rows nobody keeps: acc and fid only
      for (; t + kGroup <= stop; t += kGroup)              // one s_load burst per kGroup samples
      {
        FD dl[kGroup];
#pragma unroll
        for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl[u]);
      }
      for (; t < stop; ++t)
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
      if (t == next)
      {
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = step_wrap(s[b], dl);
        emit(x);
        next += every;
      }
      else
      {
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_wrap(s[b], dl);
      }
      ++t; c = 0;
    }
  }

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
