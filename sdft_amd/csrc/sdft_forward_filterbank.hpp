// sdft_forward_filterbank.hpp -- K1f: filterbank analysis (sdft_hip_sdft_filterbank_n), weighted band sums of |X|^2 on a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_power.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// the host's decomposition of a filterbank for the plan's tiles (logic::filterbank_layout; sdft_plan.hpp asserts the layouts agree)
struct FilterbankPiece { unsigned bin0, nbins, woff, dst; };   // bins [bin0, bin0 + nbins) of one band inside one tile, weights from woff on
                                                               // (the weights are in tile order: a tile's are one range)
constexpr int kFilterbankCache = 512;                          // weights of its tile a wave keeps in LDS (the first ones; the rest stay in memory)
struct FilterbankSplit { unsigned band, slot0, pieces; };      // a band over several tiles: workspace slots slot0 ... slot0 + pieces - 1
constexpr unsigned kFilterbankToWorkspace = 0x80000000u;       // FilterbankPiece::dst: this flag | slot, else the band

// the call-local row grid of EveryGrid plus the plan's filterbank: band b of row r of channel ch goes to
// out + ch * out_stride + r * nbands + b; the piece in slot s of a split band to ws + (ch * ws_rows + r - ws_row0) * nslots + s:
// the workspace holds the rows ws_row0 ... ws_row0 + ws_rows - 1, those of the time chunks of one launch
template <typename FD> struct FilterbankArgs
{
  FD* out;                    // [channels][rows][nbands], aligned to sizeof(FD) only
  size_t out_stride;          // elements per channel
  FD* ws;                     // [channels][ws_rows][nslots]; unused when no band is split
  size_t ws_row0, ws_rows;    // the rows the launch keeps: the first, and how many
  unsigned long long every, first;
  const FilterbankPiece* pieces;
  const unsigned* tile_piece0;        // [tiles + 1]
  const FD* weights;
  const FilterbankSplit* splits;
  unsigned nbands, nslots, nsplits;
};

// forward_power_kernel's geometry, carry-in, halo, window taps, time loop and state write-back.  On a kept row the wave has
// fl(fl(re * re) + fl(im * im)) of its owned bins in registers; they go to a wave-private strip of LDS, and the lanes take the
// tile's pieces in rounds of 64, each lane walking its piece in ascending bin order: s = fl(w0 p0), s = fl(s + fl(w1 p1)), ...
// A piece that is a whole band is stored to `out`, a piece of a split band to its workspace slot; filterbank_rows_kernel adds
// those.  A tile that forms no piece keeps no row and only steps the recurrence.  No cross-wave synchronisation, no workgroup
// barrier: the strip is the wave's own.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_filterbank_kernel(ForwardArgs<FD> a, FilterbankArgs<FD> g)
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
  // tile -> pieces (logic::filterbank_layout): the tile's owned bins start at own0; it forms pieces [tp0, tp1)
  const unsigned own0 = tile * a.interior_lanes * BPL;
  const unsigned tp0 = g.tile_piece0[tile], tp1 = g.tile_piece0[tile + 1];
  const bool emits = tp1 > tp0;
  // the wave's strip of LDS: the powers of its owned bins of one row.  Only this wave touches it, and a wave's LDS operations
  // complete in order: a compiler-level fence orders them, no barrier is needed
  __shared__ FD strips[kWavesPerBlock][kWave * BPL];
  FD* const strip = strips[wib];
  const int cell = (lane - HL) * BPL;                      // of the lane's first bin in the strip (owner lanes only)
  // the lane's piece of the first round stays in registers for the whole chunk (most tiles have fewer than 64 pieces)
  FilterbankPiece mine = {0u, 0u, 0u, 0u};
  if (tp0 + (unsigned)lane < tp1) mine = g.pieces[tp0 + (unsigned)lane];
  // the first kFilterbankCache weights of the tile go to LDS once per chunk (a mel or octave filterbank fits whole): a piece's walk
  // is a chain of dependent additions, and its operands should not come from memory row after row
  __shared__ FD caches[kWavesPerBlock][kFilterbankCache];
  FD* const cache = caches[wib];
  unsigned tw0 = 0, twn = 0;                               // the tile's first weight, and how many are cached
  if (emits)
  {
    const FilterbankPiece head = g.pieces[tp0], tail = g.pieces[tp1 - 1];
    tw0 = head.woff;
    twn = tail.woff + tail.nbins - tw0;
    if (twn > (unsigned)kFilterbankCache) twn = (unsigned)kFilterbankCache;
    for (unsigned i = (unsigned)lane; i < twn; i += kWave) cache[i] = g.weights[tw0 + i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  BinState<FD> s[BPL];
  bool flip[BPL], live[BPL], own[BPL];
  const size_t cbase = (ch * a.chunks + chunk) * a.nbins;
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    const long kk = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
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
  size_t row = emits ? (next - first) / every : 0;
  if (!emits) next = ~(size_t)0;
  FD* const out = g.out + ch * g.out_stride;
  FD* const ws = g.ws + ch * g.ws_rows * (size_t)g.nslots;

  // the weighted sum of a piece, in ascending bin order: every product rounded once, then added (no fused multiply-add)
  auto piece_sum = [&](const FilterbankPiece& pc) __attribute__((always_inline))
  {
    const FD* sp = strip + (pc.bin0 - own0);
    // (four terms' operands in flight; the additions stay in bin order)
    auto walk = [&](auto wp) __attribute__((always_inline))
    {
      FD acc = wp[0] * sp[0];
      unsigned j = 1;
      for (; j + 4 <= pc.nbins; j += 4)
      {
        const FD w0 = wp[j], w1 = wp[j + 1], w2 = wp[j + 2], w3 = wp[j + 3];
        const FD p0 = sp[j], p1 = sp[j + 1], p2 = sp[j + 2], p3 = sp[j + 3];
        const FD t0 = w0 * p0, t1 = w1 * p1, t2 = w2 * p2, t3 = w3 * p3;
        acc = acc + t0; acc = acc + t1; acc = acc + t2; acc = acc + t3;
      }
      for (; j < pc.nbins; ++j)
      {
        const FD term = wp[j] * sp[j];
        acc = acc + term;
      }
      return acc;
    };
    const unsigned rel = pc.woff - tw0;
    const FD sum = rel + pc.nbins <= twn ? walk(cache + rel) : walk(g.weights + pc.woff);
    if (pc.dst & kFilterbankToWorkspace) ws[(row - g.ws_row0) * (size_t)g.nslots + (pc.dst & ~kFilterbankToWorkspace)] = sum;
    else out[row * (size_t)g.nbands + pc.dst] = sum;
  };

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

    // the row's powers to the strip, then lanes take the tile's pieces in rounds of 64
    __builtin_amdgcn_wave_barrier();                       // (the previous row's reads are done)
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (own[b]) strip[cell + b] = p[b];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (mine.nbins) piece_sum(mine);
    for (unsigned i = tp0 + kWave + (unsigned)lane; i < tp1; i += kWave) piece_sum(g.pieces[i]);
    ++row;
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


// The split bands, after a forward launch on the same stream.  One thread per (channel, row of the launch, split band): it adds
// the band's pieces in ascending tile order -- a fixed order, so the result depends on nothing but the pieces -- and stores the band.
template <typename FD>
__global__ __launch_bounds__(kBlock) void filterbank_rows_kernel(FilterbankArgs<FD> g, unsigned channels)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned s = (unsigned)(i % g.nsplits);
  const unsigned long long rest = i / g.nsplits;
  const size_t row = (size_t)(rest % g.ws_rows);
  const size_t ch = (size_t)(rest / g.ws_rows);
  if (ch >= channels) return;
  const FilterbankSplit sp = g.splits[s];
  const FD* w = g.ws + (ch * g.ws_rows + row) * (size_t)g.nslots + sp.slot0;
  FD sum = w[0];
  for (unsigned j = 1; j < sp.pieces; ++j) sum = sum + w[j];
  g.out[ch * g.out_stride + (g.ws_row0 + row) * (size_t)g.nbands + sp.band] = sum;
}

}  // namespace sdfthip
