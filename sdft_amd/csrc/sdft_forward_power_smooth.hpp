// sdft_forward_power_smooth.hpp -- K1o: smoothed power analysis (sdft_hip_sdft_power_smooth_n), the one-pole average
// s[t] = fl(fl(a * s[t - 1]) + fl(b * |X[t]|^2)) of a band of bins, kept on a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_power_sum.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// Bin k of the row of grid point first + r * every of channel ch goes to out + ch * out_stride + r * nbins_out + (k - bin0).
// state_in: [channels][nbins_out], s before the call's first sample (chunk 0 reads it); state_out: s after its last -- written by
// the forward kernel in a call of one chunk (ends == nullptr), by smooth_scan_kernel otherwise.  They are two buffers, so that a
// call that is run again (Plan::forward_device) starts from the same values.
// ends: the workspace [channels][chunks][nbins_out] (logic::power_smooth_slot) of a call of more than one chunk: the forward kernel
// leaves E_c there, the value its chunk ends with (chunk 0 from the incoming state, every later chunk from +0); smooth_scan_kernel
// replaces E_c by S_c, the true s before the chunk's first sample.
// pw: P[j] = fl(a^j), j = 0 ... chunk_len (logic::power_smooth_table); the forward kernel does not read it.
template <typename FD> struct PowerSmoothArgs
{
  FD* out;                    // [channels][rows][nbins_out], aligned to sizeof(FD) only; nullptr: the call keeps no row
  size_t out_stride;          // elements per channel
  const FD* state_in;         // never nullptr (the plan's buffers)
  FD* state_out;
  FD* ends;                   // nullptr for a call of one chunk
  const FD* pw;               // likewise
  FD a, b;                    // the rounded decay and fl(1 - a)
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// forward_pooled_power_kernel (geometry, carry-in, halo, window taps, band test, emits, bursts of kGroup, the roll-over step, the
// state write-back) with a recursion for the sum: the term p = fl(fl(re * re) + fl(im * im)) of EVERY sample enters the
// accumulator as s = fl(fl(a * s) + fl(b * p)), no fused multiply-add.  At a grid point the accumulator is stored AFTER that
// sample's step (`next` is the sample after the grid point: the store happens on the way into it) and is not cleared.  Chunk 0
// starts from the incoming state, every later chunk from +0: the recursion is linear, so what such a chunk leaves out is
// a^(samples into the chunk) * (s before the chunk), which smooth_fix_kernel adds once smooth_scan_kernel knows it.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_power_smooth_kernel(ForwardArgs<FD> a, PowerSmoothArgs<FD> g)
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
    sm[b] = (chunk == 0 && keep[b]) ? g.state_in[ch * (size_t)g.nbins_out + (size_t)(k - band0)] : (FD)0;
  }

  const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
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

  // the grid point t - 1 has been stepped: its row goes out, the accumulator stays
  auto store_row = [&]() __attribute__((always_inline))
  {
    FD* dst = g.out + ch * g.out_stride + row * (size_t)g.nbins_out + (kfirst - band0);
    if constexpr (BPL == 2)
    {
      if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 7u) == 0)
      {
        using V = typename StoreVec<FD, 1>::type;
        V v; v.x = sm[0]; v.y = sm[1];
        store_vec(reinterpret_cast<V*>(dst), v);
      }
      else
      {
        if (keep[0]) dst[0] = sm[0];
        if (keep[1]) dst[1] = sm[1];
      }
    }
    else
    {
      if (keep[0]) dst[0] = sm[0];
    }
    ++row; next += every;
  };

  auto smooth = [&](cx<FD> (&x)[BPL]) __attribute__((always_inline))
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
        if (t == next) store_row();
        const size_t stop = next < end ? next : end;       // the samples up to the next grid point, before the roll-over
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
            smooth(x);
          }
        }
        for (; t < stop; ++t)
        {
          const FD dl = d[t];
          cx<FD> x[BPL];
#pragma unroll
          for (int b = 0; b < BPL; ++b) x[b] = step_normal(s[b], dl);
          smooth(x);
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
        if (t == next) store_row();
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = step_wrap(s[b], dl);
        smooth(x);
      }
      else
      {
#pragma unroll
        for (int b = 0; b < BPL; ++b) advance_wrap(s[b], dl);
      }
      ++t; c = 0;
    }
  }
  if (emits)
  {
    if (t1 == next) store_row();                           // the chunk's last sample is a grid point
    // what the chunk ends with: E_c for the scan, or -- a call of one chunk -- the state itself
    FD* const endp = g.ends ? g.ends + (ch * a.chunks + chunk) * (size_t)g.nbins_out : g.state_out + ch * (size_t)g.nbins_out;
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (keep[b]) endp[kfirst + b - band0] = sm[b];
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


// The carry across time chunks, after the forward launches of the call on the same stream (chunks > 1).  One thread per (channel,
// bin of the band) walks the chunks in ascending order: S_1 = E_0, S_{c + 1} = fl(fl(P[len_c] * S_c) + E_c), len_c the samples of
// chunk c.  It leaves S_c in the place of E_c (c >= 1: slot 0 keeps E_0 and is not read again) and the last value in state.  The
// loads go kGroup at a time, as pooled_power_rows_kernel's; only the arithmetic is serial.
template <typename FD>
__global__ __launch_bounds__(kBlock) void smooth_scan_kernel(PowerSmoothArgs<FD> g, size_t n, unsigned chunks, unsigned chunk_len, unsigned chunk_shift,
                                                            unsigned channels)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned k = (unsigned)(i % g.nbins_out);
  const size_t ch = (size_t)(i / g.nbins_out);
  if (ch >= channels) return;
  FD* const e = g.ends + ch * chunks * (size_t)g.nbins_out + k;
  const FD pfull = g.pw[chunk_len];                          // every chunk but the first and the last has chunk_len samples
  auto len = [&](size_t c) -> size_t
  {
    const size_t t0 = c * chunk_len - chunk_shift, tn = t0 + chunk_len;
    return (tn < n ? tn : n) - t0;
  };
  FD s = e[0];
  size_t c = 1;
  for (; c + kGroup < chunks; c += kGroup)                   // whole chunks only: the last one has its own length
  {
    FD v[kGroup];
#pragma unroll
    for (int u = 0; u < kGroup; ++u) v[u] = e[(c + u) * (size_t)g.nbins_out];
#pragma unroll
    for (int u = 0; u < kGroup; ++u)
    {
      e[(c + u) * (size_t)g.nbins_out] = s;
      const FD ps = pfull * s;
      s = ps + v[u];
    }
  }
  for (; c < chunks; ++c)
  {
    const FD v = e[c * (size_t)g.nbins_out];
    e[c * (size_t)g.nbins_out] = s;
    const FD ps = g.pw[len(c)] * s;
    s = ps + v;
  }
  g.state_out[ch * (size_t)g.nbins_out + k] = s;
}

// What the chunks c >= 1 left out of their rows, after smooth_scan_kernel.  One thread per (channel, kept row, bin of the band):
// the row of sample t in chunk c >= 1 (logic::power_smooth_fix) becomes fl(row + fl(P[t - t0_c + 1] * S_c)).
template <typename FD>
__global__ __launch_bounds__(kBlock) void smooth_fix_kernel(PowerSmoothArgs<FD> g, size_t rows, unsigned chunks, unsigned chunk_len, unsigned chunk_shift,
                                                           unsigned channels)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned k = (unsigned)(i % g.nbins_out);
  const unsigned long long rest = i / g.nbins_out;
  const size_t row = (size_t)(rest % rows);
  const size_t ch = (size_t)(rest / rows);
  if (ch >= channels) return;
  const size_t t = (size_t)g.first + row * (size_t)g.every;
  const size_t c = (t + chunk_shift) / chunk_len;
  if (c == 0) return;
  const size_t t0 = c * chunk_len - chunk_shift;
  const FD sc = g.ends[(ch * chunks + c) * (size_t)g.nbins_out + k];
  FD* const dst = g.out + ch * g.out_stride + row * (size_t)g.nbins_out + k;
  const FD ps = g.pw[t - t0 + 1] * sc;
  *dst = *dst + ps;
}

}  // namespace sdfthip
