// sdft_forward_band_peak.hpp -- K1b: band-peak analysis (sdft_hip_sdft_band_peak_n), the largest weighted |X|^2 of a band and its bin on a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_filterbank.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// The call reads the plan's filterbank through forward_filterbank_kernel's tables (FilterbankPiece, tile_piece0, FilterbankSplit,
// the weights in tile order) and takes its arguments in FilterbankArgs, read with two numbers where that call has one: band b of
// row r of channel ch goes to the PAIR at out + ch * out_stride + (r * nbands + b) * 2 -- [0] the value, [1] the absolute bin as a
// number of FD -- and the piece in slot s of a split band to the pair at ws + ((ch * ws_rows + r - ws_row0) * nslots + s) * 2.

// The rule, of a held pair (m, i) and a candidate v at a HIGHER bin: the candidate is taken when it is larger, or when it is the
// first NaN.  Strict, so the lowest bin of the largest value stays, a NaN stays once held, and equal zeros of either sign keep
// the first one's bits: np.argmax's choice (logic::band_peak_take is the host's restatement).
// Evaluated here as  m == m  and  not (v <= m)  -- the same truth table: a held NaN takes nothing; otherwise v <= m is false
// exactly for a larger v and for a NaN -- with a bitwise and, so that a walk is compares and selects, no branch.
template <typename FD> __device__ __forceinline__ bool band_peak_take(FD m, FD v) { return (m == m) & !(v <= m); }

// a pair to memory aligned to sizeof(FD) only: one vector store where the pair is aligned, else two scalar stores (the moments
// kernel's rule for its pairs)
template <typename FD> __device__ __forceinline__ void band_peak_store(FD* q, FD value, FD bin)
{
  if ((reinterpret_cast<size_t>(q) & (2 * sizeof(FD) - 1)) == 0)
  {
    using V = typename StoreVec<FD, 1>::type;
    V v; v.x = value; v.y = bin;
    store_vec(reinterpret_cast<V*>(q), v);
  }
  else { q[0] = value; q[1] = bin; }
}

// forward_filterbank_kernel's geometry, carry-in, halo, window taps, time loop, state write-back, wave-private strip and LDS
// weight cache.  On a kept row the lanes take the tile's pieces in rounds of 64, each lane walking its piece in ascending bin
// order with the rule above: (m, i) = (fl(w0 p0), bin0), then every later v = fl(w p) -- one rounded product, no fused
// multiply-add -- against the held pair.  A piece that is a whole band stores its pair to `out`, a piece of a split band to its
// workspace slot; band_peak_rows_kernel joins those by the same rule.  A tile that forms no piece keeps no row and only steps
// the recurrence.  No cross-wave synchronisation, no workgroup barrier, no atomics: the strip is the wave's own.
template <typename FD, int BPL, int WIN>
__global__ __launch_bounds__(kBlock) void forward_band_peak_kernel(ForwardArgs<FD> a, FilterbankArgs<FD> g)
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
  // is a chain of compares and selects on the held pair, and its operands should not come from memory row after row
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
  FD* const ws = g.ws + ch * g.ws_rows * (size_t)g.nslots * 2;

  // the peak of a piece, in ascending bin order: every product rounded once, then compared (no fused multiply-add)
  auto piece_peak = [&](const FilterbankPiece& pc) __attribute__((always_inline))
  {
    const FD* sp = strip + (pc.bin0 - own0);
    // (four candidates' operands in flight; the comparisons stay in bin order)
    auto walk = [&](auto wp, unsigned& at) __attribute__((always_inline))
    {
      FD best = wp[0] * sp[0];
      at = 0;
      auto take = [&](FD v, unsigned j) __attribute__((always_inline))
      {
        const bool t = band_peak_take(best, v);
        best = t ? v : best; at = t ? j : at;
      };
      unsigned j = 1;
      for (; j + 4 <= pc.nbins; j += 4)
      {
        const FD w0 = wp[j], w1 = wp[j + 1], w2 = wp[j + 2], w3 = wp[j + 3];
        const FD p0 = sp[j], p1 = sp[j + 1], p2 = sp[j + 2], p3 = sp[j + 3];
        const FD v0 = w0 * p0, v1 = w1 * p1, v2 = w2 * p2, v3 = w3 * p3;
        take(v0, j); take(v1, j + 1); take(v2, j + 2); take(v3, j + 3);
      }
      for (; j < pc.nbins; ++j) take(wp[j] * sp[j], j);
      return best;
    };
    const unsigned rel = pc.woff - tw0;
    unsigned at;
    const FD best = rel + pc.nbins <= twn ? walk(cache + rel, at) : walk(g.weights + pc.woff, at);
    const FD bin = (FD)(pc.bin0 + at);
    if (pc.dst & kFilterbankToWorkspace)
    {
      // (the workspace is the plan's own allocation: its pairs are aligned)
      FD* const q = ws + ((row - g.ws_row0) * (size_t)g.nslots + (pc.dst & ~kFilterbankToWorkspace)) * 2;
      q[0] = best; q[1] = bin;
    }
    else band_peak_store(out + (row * (size_t)g.nbands + pc.dst) * 2, best, bin);
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
    if (mine.nbins) piece_peak(mine);
    for (unsigned i = tp0 + kWave + (unsigned)lane; i < tp1; i += kWave) piece_peak(g.pieces[i]);
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


// The split bands, after a forward launch on the same stream.  One thread per (channel, row of the launch, split band): it joins
// the band's pieces in ascending tile order by the rule -- the lower piece is the held pair, the higher one the candidate, so a
// tie across a tile boundary keeps the lower bin -- and stores the band's pair.
template <typename FD>
__global__ __launch_bounds__(kBlock) void band_peak_rows_kernel(FilterbankArgs<FD> g, unsigned channels)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned s = (unsigned)(i % g.nsplits);
  const unsigned long long rest = i / g.nsplits;
  const size_t row = (size_t)(rest % g.ws_rows);
  const size_t ch = (size_t)(rest / g.ws_rows);
  if (ch >= channels) return;
  const FilterbankSplit sp = g.splits[s];
  const FD* w = g.ws + ((ch * g.ws_rows + row) * (size_t)g.nslots + sp.slot0) * 2;
  FD best = w[0], bin = w[1];
  for (unsigned j = 1; j < sp.pieces; ++j)
  {
    const FD v = w[2 * j], at = w[2 * j + 1];
    const bool t = band_peak_take(best, v);
    best = t ? v : best; bin = t ? at : bin;
  }
  band_peak_store(g.out + ch * g.out_stride + ((g.ws_row0 + row) * (size_t)g.nbands + sp.band) * 2, best, bin);
}

}  // namespace sdfthip
