// sdft_forward_smooth_peak.hpp -- K1os: smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n), the largest or the smallest of the
// one-pole average s[t] = fl(fl(a * s[t - 1]) + fl(b * |X[t]|^2)) of a band of bins over the windows of a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_power_peak.hpp"
#include "sdft_forward_power_smooth.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// rows: the peak-hold call's arguments as they are (the grid, the windows, the head row, the output and the workspace of cut
// windows); peak_rows_kernel takes them unchanged.
// state_in: [channels][nbins_out], s before the call's first sample (chunk 0 reads it); state_out: s after its last, written by
// the last chunk.  Two buffers, so that a call that is run again (Plan::forward_device) starts from the same values.
// ends: [channels][chunks][nbins_out] (logic::power_smooth_slot) of a call of more than one chunk: S_c, the value of s before the
// first sample of chunk c >= 1, as smooth_scan_kernel left it after the carry pass; slot 0 is not read.
template <typename FD> struct SmoothPeakArgs
{
  PowerSumArgs<FD> rows;
  const FD* state_in;         // never nullptr (the plan's buffers)
  FD* state_out;
  const FD* ends;             // nullptr for a call of one chunk
  FD a, b;                    // the rounded decay and fl(1 - a)
};

// forward_power_peak_kernel (geometry, carry-in, halo, window taps, band test, bursts of kGroup, the roll-over step, the flush
// rule at window boundaries, slot 0 / slot 1 of the cut-window workspace, the state write-back) with
// forward_power_smooth_kernel's recursion in the loop: the term p = fl(fl(re * re) + fl(im * im)) of EVERY sample enters
// sm = fl(fl(a * sm) + fl(b * p)), no fused multiply-add, and sm AFTER that step goes into the window's accumulator by peak_hold.
// A flush leaves the accumulator at peak_start and sm as it is.  Chunk 0 starts sm from the incoming state, every chunk c >= 1
// from S_c -- the carries come before the rows, because the extreme of s0[t] + a^j * S_c over a window is not a function of the
// extreme of s0[t] -- so every value held is the sequential recursion from S_c.  The last chunk leaves sm in state_out.
template <typename FD, int BPL, int WIN, int HOLD>
__global__ __launch_bounds__(kBlock) void forward_smooth_peak_kernel(ForwardArgs<FD> a, SmoothPeakArgs<FD> q)
{
  constexpr int H = win_halo<WIN>::value;                 // halo bins per side
  constexpr int HL = (H + BPL - 1) / BPL;                 // halo lanes per side
  const PowerSumArgs<FD>& g = q.rows;

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
  // s before the chunk's first sample: the incoming state, or S_c
  const FD* const start = chunk == 0 ? q.state_in + ch * (size_t)g.nbins_out : q.ends + (ch * a.chunks + chunk) * (size_t)g.nbins_out;
  FD sm[BPL];                                              // the smoothed power of the lane's bins
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
    sm[b] = keep[b] ? start[(size_t)(k - band0)] : (FD)0;
  }

  const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
  const FD w = a.wscale;
  const FD ca = q.a, cb = q.b;
  const bool last_chunk = (chunk + 1 == a.chunks);

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
  FD held[BPL];
#pragma unroll
  for (int b = 0; b < BPL; ++b) held[b] = peak_start<FD>(HOLD);

  // the window's samples of this chunk end at sample t (exclusive): a whole row, or a piece for the workspace
  auto flush = [&](size_t t) __attribute__((always_inline))
  {
    const size_t wend = next < a.n ? next : a.n;
    FD* dst;
    if (!cut && t == wend) dst = row ? g.rest + ch * g.rest_stride + (row - 1) * (size_t)g.nbins_out : g.row0 + ch * g.row0_stride;
    else dst = g.ws + ((ch * a.chunks + chunk) * 2 + (cut ? 0 : 1)) * (size_t)g.nbins_out;
    dst += kfirst - band0;
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 7u) == 0)
      {
        using V = typename StoreVec<FD, 1>::type;
        V v; v.x = held[0]; v.y = held[1];
        store_vec(reinterpret_cast<V*>(dst), v);
      }
      else
      {
        if (keep[0]) dst[0] = held[0];
        if (keep[1]) dst[1] = held[1];
      }
    }
    else
    {
      if (keep[0]) dst[0] = held[0];
    }
#pragma unroll
    for (int b = 0; b < BPL; ++b) held[b] = peak_start<FD>(HOLD);
    ++row; next += every; cut = false;
  };

  auto hold = [&](cx<FD> (&x)[BPL]) __attribute__((always_inline))
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
      const FD as = ca * sm[b], bp = cb * p;
      sm[b] = as + bp;
      held[b] = peak_hold(held[b], sm[b], HOLD);
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
            hold(x);
          }
        }
        for (; t < stop; ++t)
        {
          const FD dl = d[t];
          cx<FD> x[BPL];
#pragma unroll
          for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl);
          hold(x);
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
        hold(x);
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
    FD* const endp = q.state_out + ch * (size_t)g.nbins_out;
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      if (keep[b]) endp[kfirst + b - band0] = sm[b];       // s after the call's last sample
      if (own[b])
      {
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
    }
  }
}

}  // namespace sdfthip
