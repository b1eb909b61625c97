// sdft_forward_every.hpp -- K1e: decimated analysis (sdft_hip_sdft_every_n), only every `every`-th row of the matrix is formed
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp); citations are into /root/reference/c/src/sdft/sdft.h.

#pragma once

#include "sdft_forward.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// the call-local row grid: rows at the call's samples first, first + every, ... < n; row r of channel ch goes to
// ForwardArgs::out + ch * out_stride + r * N
struct EveryGrid
{
  unsigned long long every, first;
};

// forward_kernel's geometry (lanes are bins, independent tiles with halo lanes: any N, no LDS) and carry-in, but the time
// loop does the reference's step on acc and fid only (sdft.h:572-574, :583-584) -- the demodulation (:585), the mirror,
// the window and the row store only at the grid's samples.  The state arithmetic is the same operation for operation, so
// the state after the call and every kept row are what sdft_sdft_n gives them.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_every_kernel(ForwardArgs<FD> a, EveryGrid g)
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

  BinState<FD> s[BPL];
  bool flip[BPL], live[BPL], keep[BPL];
  const size_t cbase = (ch * a.chunks + chunk) * a.nbins;
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    const long kk = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    keep[b] = owner && k >= 0 && k < nbins;
    s[b].tw = a.tw[kk];
    s[b].acc = a.carry[cbase + kk];
    s[b].fid = a.fseed ? fid_from_table(a.fseed, a.fseed_L, a.nbins, kk, c, s[b].tw)
             : a.seed  ? a.seed[cbase + kk] : a.wtab[(size_t)(((unsigned long long)kk * c) % span)];
  }

  const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
  const FD w = a.wscale;
  const bool last_chunk = (chunk + 1 == a.chunks);

  // the chunk's first grid sample and its row (wave-uniform; one division per wave)
  const size_t every = (size_t)g.every, first = (size_t)g.first;
  size_t next = first;
  if (t0 > first) next = first + ((t0 - first + every - 1) / every) * every;
  cx<FD>* dst = a.out + ch * a.out_stride + ((next - first) / every) * (size_t)a.nbins + kfirst;

  auto emit = [&](cx<FD> (&x)[BPL])
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
    cx<FD> y[BPL];
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      y[b] = window_tap<FD, WIN>(e[b], e[b + 1], e[b + 2], e[b + 3], e[b + 4], w);

    if constexpr (BPL == 2)
    {
      if (a.vec_store)
      {
        if (keep[0])
        {
          using V = typename StoreVec<FD, 2>::type;
          V v; v.x = y[0].re; v.y = y[0].im; v.z = y[1].re; v.w = y[1].im;
          store_vec(reinterpret_cast<V*>(dst), v);
        }
      }
      else
      {
        if (keep[0]) dst[0] = y[0];
        if (keep[1]) dst[1] = y[1];
      }
    }
    else
    {
      if (keep[0])
      {
        using V = typename StoreVec<FD, 1>::type;
        V v; v.x = y[0].re; v.y = y[0].im;
        store_vec(reinterpret_cast<V*>(dst), v);
      }
    }
    dst += a.nbins;
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
      if (keep[b])
      {
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
  }
}

}  // namespace sdfthip
