// sdft_forward_power_peak.hpp -- K1k: peak-hold analysis (sdft_hip_sdft_power_peak_n), the largest or the smallest |X|^2 of a band
// of bins over the windows of a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_power_sum.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

constexpr int kHoldMax = 0, kHoldMin = 1;                   // enum sdft_hip_hold

// The combining rule (logic::peak_hold is the same function for the host): the extreme of the held value m and the term p; a NaN
// term takes the place of whatever is held and no later term replaces it (every comparison with it is false), so a window with a
// NaN term gives NaN.  Without one the result is one of the terms, bit for bit: max and min are associative and commutative, so
// how chunks and segments cut a window does not show.
template <typename FD> __device__ __forceinline__ FD peak_hold(FD m, FD p, int hold)
{
  return hold == kHoldMin ? ((p < m || p != p) ? p : m) : ((p > m || p != p) ? p : m);
}
// what an empty accumulator holds: every window and every piece of one has a sample, so it never reaches the output
template <typename FD> __device__ __forceinline__ FD peak_start(int hold)
{
  return hold == kHoldMin ? (FD)__builtin_huge_val() : -(FD)__builtin_huge_val();
}

// forward_pooled_power_kernel (geometry, carry-in, halo, window taps, band test, bursts of kGroup, flush rule, state write-back;
// PowerSumArgs as they are: the grid, the windows, the head row, the output and the workspace of cut windows) with the other
// statistic: the term fl(fl(re * re) + fl(im * im)) of every sample goes into the accumulator by peak_hold, and a flush leaves
// the accumulator at peak_start.  Pieces of cut windows go to slot 0 or 1 of the chunk's workspace; peak_rows_kernel combines them.
template <typename FD, int BPL, int WIN, int HOLD>
__global__ __launch_bounds__(kBlock) void forward_power_peak_kernel(ForwardArgs<FD> a, PowerSumArgs<FD> g)
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
      held[b] = peak_hold(held[b], p, HOLD);
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
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (own[b])
      {
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
  }
}


// pooled_power_rows_kernel's twin: the rows a chunk boundary cuts, after the forward launches of the call on the same stream.  One
// thread per (channel, chunk c >= 1, bin of the band).  If a window runs across the start of chunk c and began in chunk c - 1, the
// thread combines the window's pieces -- slot 1 of chunk c - 1, then slot 0 of the chunks c, c + 1, ... the window reaches
// (logic::power_sum_row_chunks) -- by peak_hold and stores the row.
template <typename FD>
__global__ __launch_bounds__(kBlock) void peak_rows_kernel(PowerSumArgs<FD> g, size_t n, unsigned chunks, unsigned chunk_len, unsigned chunk_shift,
                                                          unsigned channels, int hold)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned k = (unsigned)(i % g.nbins_out);
  const unsigned long long rest = i / g.nbins_out;
  const size_t c = 1 + (size_t)(rest % (chunks - 1u));
  const size_t ch = (size_t)(rest / (chunks - 1u));
  if (ch >= channels) return;
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  const size_t t0 = c * chunk_len - chunk_shift;
  // the window of sample t0 (t0 < n: the chunk exists)
  size_t row = 0, begin = 0, end = first;
  if (t0 >= first)
  {
    const size_t j = (t0 - first) / every;
    row = (first > 0 ? 1 : 0) + j;
    begin = first + j * every;
    end = every < n - begin ? begin + every : n;
  }
  if (end > n) end = n;
  if (begin == t0) return;                                 // a window starts with the chunk: nothing is cut here
  const size_t c0 = (begin + chunk_shift) / chunk_len, c1 = (end - 1 + chunk_shift) / chunk_len;
  if (c0 + 1 != c) return;                                 // the row of an earlier thread
  const FD* ws = g.ws + ch * chunks * 2 * (size_t)g.nbins_out + k;
  FD s = ws[(c0 * 2 + 1) * (size_t)g.nbins_out];
  size_t cc = c;
  for (; cc + kGroup <= c1 + 1; cc += kGroup)               // a window over many chunks: kGroup loads in flight
  {
    FD v[kGroup];
#pragma unroll
    for (int u = 0; u < kGroup; ++u) v[u] = ws[((cc + u) * 2) * (size_t)g.nbins_out];
#pragma unroll
    for (int u = 0; u < kGroup; ++u) s = peak_hold(s, v[u], hold);
  }
  for (; cc <= c1; ++cc) s = peak_hold(s, ws[(cc * 2) * (size_t)g.nbins_out], hold);
  FD* dst = row ? g.rest + ch * g.rest_stride + (row - 1) * (size_t)g.nbins_out : g.row0 + ch * g.row0_stride;
  dst[k] = s;
}

// pooled_power_add_kernel's twin, a call in segments on device memory: the head row of a later segment (kept apart,
// PowerSumArgs::row0) completes the row the segment before it ended with -- row[ch][k] = peak_hold(row[ch][k], head[ch][k])
template <typename FD>
__global__ __launch_bounds__(kBlock) void peak_join_kernel(FD* row, size_t row_stride, const FD* head, unsigned nbins_out, unsigned channels, int hold)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned k = (unsigned)(i % nbins_out);
  const size_t ch = (size_t)(i / nbins_out);
  if (ch >= channels) return;
  row[ch * row_stride + k] = peak_hold(row[ch * row_stride + k], head[ch * (size_t)nbins_out + k], hold);
}

}  // namespace sdfthip
