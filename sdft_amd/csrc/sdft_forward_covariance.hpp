// sdft_forward_covariance.hpp -- K1v: array covariance analysis (sdft_hip_sdft_covariance_n), A conj(B) of the windowed bins of ALL
// pairs of the channels of an array, by register blocks of G x G pairs, summed over the windows of a row grid
// Part of the kernel source of libsdft_hip.so (see sdft_kernels.hpp).

#pragma once

#include "sdft_forward_cross_sum.hpp"

#pragma clang fp contract(off)

namespace sdfthip {

// channels of a group = side of a register block, per FD type (measured: profiles/covariance_rates.txt).  A build with
// -DSDFT_HIP_TEST_HOOKS also holds the other candidates, for scripts/covariance_rates.py (option "array_group").
template <typename FD> struct cov_group { static constexpr int value = 4; };

// One work item of a covariance call (logic::covariance_items).  A block item (block != 0) has the array elements a0 ... a0 + na - 1
// on side A and b0 ... b0 + nb - 1 on side B, a0 <= b0; a0 == b0 is a diagonal block: one group, stepped once, whose pairs are the
// slots (sa <= sb), and the one item that writes the state of its channels back (writes != 0).  Another item (block == 0) only
// advances the PLAN channel a0, which is not in the array, and writes its state.
struct CovItem
{
  unsigned a0, b0;
  unsigned short na, nb, block, writes;
};

// CrossSumArgs with the array in place of the pair list: chan[i] is the plan channel of array element i, the pair of the elements
// (i <= j) has the output index p(i, j) = i * nch - i (i - 1) / 2 + (j - i) (logic::covariance_pair_index), and p takes the place
// of the cross-spectrum call's pair in the rows and in the workspace [npairs][chunks][2][nbins_out] complex.
template <typename FD> struct CovarianceArgs
{
  FD* row0;                   // [npairs][nbins_out] complex, aligned to sizeof(FD) only
  size_t row0_stride;
  FD* rest;                   // [npairs][rows - 1][nbins_out] complex, likewise
  size_t rest_stride;
  FD* ws;                     // nullptr for a call of one chunk
  const CovItem* items;       // [nitems]
  const unsigned* chan;       // [nch]
  unsigned nitems, nch, npairs;
  unsigned long long every, first;
  unsigned bin0, nbins_out;
};

// samples per scalar-load burst: the hot loop holds (channels of both sides) x (samples of a burst) steps, so the burst shrinks
// as the block grows (forward_cross_sum_kernel: two channels, eight samples)
template <bool B> struct cov_flag { static constexpr bool value = B; };
template <int G> struct cov_burst { static constexpr int value = G >= 4 ? 2 : (G == 2 ? 4 : 8); };

// forward_cross_sum_kernel with groups in place of channels.  A wave is (tile, chunk, item).  A block item steps the recurrences
// of the G channels of side A and, unless it is a diagonal block, of the G of side B, windows each of them ONCE per sample and
// adds the G x G terms (diagonal: the G (G + 1) / 2 with sa <= sb)
//   re = fl(fl(A.re * B.re) + fl(A.im * B.im))        im = fl(fl(A.im * B.re) - fl(A.re * B.im))
// to two accumulators per pair and bin, in time order, in FD: the cross-spectrum kernel's term, with the lower array index on
// side A, its -0 start, its windows, flushes, workspace slots (one per output index) and roll-over step -- so every element has
// that kernel's bits.  A group at the array's end with fewer than G channels is padded with the array's last channel: a padded
// slot is stepped like the others and has no output and no state to write (no guard in the hot loop).  An item that forms no row
// in this tile (a tile outside the band, an advance-only item) steps the channels it writes one after the other, without windows;
// an off-diagonal block there has nothing to do.
template <typename FD, int BPL, int WIN, int G>
__global__ __launch_bounds__(kBlock) void forward_covariance_kernel(ForwardArgs<FD> a, CovarianceArgs<FD> g)
{
  constexpr int H = win_halo<WIN>::value;                 // halo bins per side
  constexpr int HL = (H + BPL - 1) / BPL;                 // halo lanes per side
  constexpr int KB = cov_burst<G>::value;

  const int lane = threadIdx.x & (kWave - 1);
  const unsigned wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long wave = (unsigned long long)blockIdx.x * kWavesPerBlock + wib;
  if (wave >= a.total_waves) return;

  const unsigned tile = (unsigned)(wave % a.tiles);
  const unsigned long long rest = wave / a.tiles;
  const unsigned chunk = a.chunk0 + (unsigned)(rest % a.launch_chunks);
  const size_t item = (size_t)(rest / a.launch_chunks);
  if (item >= g.nitems) return;
  const SDFT_CONSTANT CovItem* its = as_uniform(g.items);
  const SDFT_CONSTANT unsigned* chan = as_uniform(g.chan);
  const unsigned a0 = its[item].a0, b0 = its[item].b0, na = its[item].na, nb = its[item].nb;
  const bool block = its[item].block != 0, writes = its[item].writes != 0;
  const bool diag = a0 == b0;                              // wave-uniform

  const long nbins = (long)a.nbins;
  const unsigned span = 2u * a.nbins, maxc = span - 1u;
  const size_t t0 = chunk ? (size_t)chunk * a.chunk_len - a.chunk_shift : 0;
  const size_t tn = (size_t)(chunk + 1) * a.chunk_len - a.chunk_shift;
  const size_t t1 = tn < a.n ? tn : a.n;
  const unsigned c0 = (unsigned)(((size_t)a.cursor0 + t0) % span);

  // lane -> bins
  const long kfirst = (long)tile * a.interior_lanes * BPL + (long)(lane - HL) * BPL;
  const bool owner = (lane >= HL) && (lane < HL + (int)a.interior_lanes);
  // tile -> band (logic::power_tile_emits): the tile's owned bins [own0, own1) against [bin0, bin0 + nbins_out)
  const long own0 = (long)tile * a.interior_lanes * BPL;
  const long own1 = own0 + (long)a.interior_lanes * BPL < nbins ? own0 + (long)a.interior_lanes * BPL : nbins;
  const long band0 = (long)g.bin0, band1 = band0 + (long)g.nbins_out;
  const bool emits = block && own0 < band1 && band0 < own1;
  if (!emits && !writes) return;

  bool flip[BPL], live[BPL], own[BPL], keep[BPL];
  long kks[BPL];
  cx<FD> tw[BPL];
#pragma unroll
  for (int b = 0; b < BPL; ++b)
  {
    const long k = kfirst + b;
    kks[b] = reflect_bin(k, nbins, flip[b]);
    live[b] = !(nbins == 1 && k != 0);                    // N == 1: halo cells are zero for ever
    own[b] = owner && k >= 0 && k < nbins;
    keep[b] = own[b] && k >= band0 && k < band1;
    tw[b] = a.tw[kks[b]];
  }
  const bool last_chunk = (chunk + 1 == a.chunks);
  // the carry-in of the chunk for one plan channel, and the channel's state from the last chunk
  auto load = [&](BinState<FD> (&s)[BPL], size_t ch) __attribute__((always_inline))
  {
    const size_t cbase = (ch * a.chunks + chunk) * a.nbins;
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      s[b].tw = tw[b];
      s[b].acc = a.carry[cbase + kks[b]];
      s[b].fid = a.fseed ? fid_from_table(a.fseed, a.fseed_L, a.nbins, kks[b], c0, tw[b])
               : a.seed  ? a.seed[cbase + kks[b]] : a.wtab[(size_t)(((unsigned long long)kks[b] * c0) % span)];
    }
  };
  auto store = [&](const BinState<FD> (&s)[BPL], size_t ch) __attribute__((always_inline))
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
      if (own[b])
      {
        a.acc_state[ch * a.nbins + kfirst + b] = s[b].acc;
        a.fid_state[ch * a.nbins + kfirst + b] = s[b].fid;
      }
  };

  if (!emits)
  {
    // no row to form: the channels this item writes, one after the other, acc and fid only
    const unsigned nadv = block ? na : 1u;
    for (unsigned q = 0; q < nadv; ++q)
    {
      const size_t ch = block ? chan[a0 + q] : a0;
      BinState<FD> s[BPL];
      load(s, ch);
      const SDFT_CONSTANT FD* d = as_uniform(a.delta + ch * a.n);
      unsigned c = c0;
      size_t t = t0;
      while (t < t1)
      {
        size_t run = maxc - c;                             // normal steps before the roll-over
        if (run > t1 - t) run = t1 - t;
        const size_t end = t + run;
        for (; t + kGroup <= end; t += kGroup)
        {
          FD dl[kGroup];
#pragma unroll
          for (int u = 0; u < kGroup; ++u) dl[u] = d[t + u];
#pragma unroll
          for (int u = 0; u < kGroup; ++u)
          {
#pragma unroll
            for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl[u]);
          }
        }
        for (; t < end; ++t)
        {
          const FD dl = d[t];
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_normal(s[b], dl);
        }
        c += (unsigned)run;
        if (t < t1)
        {
          const FD dl = d[t];
#pragma unroll
          for (int b = 0; b < BPL; ++b) advance_wrap(s[b], dl);
          ++t; c = 0;
        }
      }
      if (last_chunk) store(s, ch);
    }
    return;
  }

  // ---- a block that forms rows ----
  const unsigned top = g.nch - 1u;
  size_t cha[G], chb[G];
  BinState<FD> sa[G][BPL], sb[G][BPL];
  const SDFT_CONSTANT FD* da[G];
  const SDFT_CONSTANT FD* db[G];
#pragma unroll
  for (int s = 0; s < G; ++s)
  {
    cha[s] = chan[a0 + s < top ? a0 + s : top];            // (a padded slot: the array's last channel once more)
    chb[s] = chan[b0 + s < top ? b0 + s : top];
    load(sa[s], cha[s]);
    da[s] = as_uniform(a.delta + cha[s] * a.n);
    db[s] = as_uniform(a.delta + chb[s] * a.n);
    if (!diag) load(sb[s], chb[s]);
    else
    {
#pragma unroll
      for (int b = 0; b < BPL; ++b) sb[s][b] = sa[s][b];   // (a diagonal block has no side B: never stepped)
    }
  }
  const FD w = a.wscale;
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
  FD sre[G][G][BPL], sim[G][G][BPL];
#pragma unroll
  for (int i = 0; i < G; ++i)
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int b = 0; b < BPL; ++b) { sre[i][j][b] = (FD)-0.0; sim[i][j][b] = (FD)-0.0; }

  // the window's samples of this chunk end at sample t (exclusive): whole rows, or pieces for the workspace, of every pair of the
  // block.  A lane holds 16 bytes of a row (one double pair, two float pairs); the row is aligned to sizeof(FD) only
  auto flush = [&](size_t t) __attribute__((always_inline))
  {
    const size_t wend = next < a.n ? next : a.n;
    const bool whole = !cut && t == wend;
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
      for (int j = 0; j < G; ++j)
      {
        const bool valid = (unsigned)i < na && (unsigned)j < nb && (!diag || i <= j);      // wave-uniform
        if (valid)
        {
          const size_t ei = a0 + i, ej = b0 + j;
          const size_t p = (ei * (2 * (size_t)g.nch - ei + 1)) / 2 + (ej - ei);          // = ei * nch - ei (ei - 1) / 2 + (ej - ei)
          FD* dst;
          if (whole) dst = row ? g.rest + p * g.rest_stride + (row - 1) * nb2 : g.row0 + p * g.row0_stride;
          else dst = g.ws + ((p * a.chunks + chunk) * 2 + (cut ? 0 : 1)) * nb2;
          dst += 2 * (kfirst - band0);
          bool done = false;
          if constexpr (BPL == 2)
          {
            if (keep[0] && keep[1] && (reinterpret_cast<size_t>(dst) & 15u) == 0)
            {
              using V = typename StoreVec<FD, 2>::type;
              V v; v.x = sre[i][j][0]; v.y = sim[i][j][0]; v.z = sre[i][j][1]; v.w = sim[i][j][1];
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
                V v; v.x = sre[i][j][b]; v.y = sim[i][j][b];
                store_vec(reinterpret_cast<V*>(q), v);
              }
              else { q[0] = sre[i][j][b]; q[1] = sim[i][j][b]; }
            }
          }
        }
#pragma unroll
        for (int b = 0; b < BPL; ++b) { sre[i][j][b] = (FD)-0.0; sim[i][j][b] = (FD)-0.0; }
      }
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
  auto add = [&](const cx<FD> (&ya)[BPL], const cx<FD> (&yb)[BPL], FD (&re_sum)[BPL], FD (&im_sum)[BPL]) __attribute__((always_inline))
  {
#pragma unroll
    for (int b = 0; b < BPL; ++b)
    {
      const FD rr = ya[b].re * yb[b].re, ii = ya[b].im * yb[b].im;
      const FD ir = ya[b].im * yb[b].re, ri = ya[b].re * yb[b].im;
      const FD re = rr + ii, im = ir - ri;
      re_sum[b] = re_sum[b] + re;
      im_sum[b] = im_sum[b] + im;
    }
  };
  // The time loop, once per kind of block (DIAG is a compile-time flag: two code paths that share no branch inside the unrolled
  // body, so the accumulators stay in registers).  One sample of the window: side A's recurrences and windows, then side B channel
  // by channel, each with its column of terms; a diagonal block has no side B -- its columns are side A's bins and end at the diagonal
  auto run = [&](auto kind) __attribute__((always_inline))
  {
    constexpr bool DIAG = decltype(kind)::value;
    auto pool = [&](const FD (&dla)[G], const FD (&dlb)[G], const bool wrap) __attribute__((always_inline))
    {
      cx<FD> ya[G][BPL];
#pragma unroll
      for (int s = 0; s < G; ++s)
      {
        cx<FD> x[BPL];
#pragma unroll
        for (int b = 0; b < BPL; ++b) x[b] = wrap ? step_wrap(sa[s][b], dla[s]) : step_normal(sa[s][b], dla[s]);
        taps(x, ya[s]);
      }
#pragma unroll
      for (int j = 0; j < G; ++j)
      {
        if constexpr (DIAG)
        {
#pragma unroll
          for (int i = 0; i <= j; ++i) add(ya[i], ya[j], sre[i][j], sim[i][j]);
        }
        else
        {
          cx<FD> x[BPL], yb[BPL];
#pragma unroll
          for (int b = 0; b < BPL; ++b) x[b] = wrap ? step_wrap(sb[j][b], dlb[j]) : step_normal(sb[j][b], dlb[j]);
          taps(x, yb);
#pragma unroll
          for (int i = 0; i < G; ++i) add(ya[i], yb, sre[i][j], sim[i][j]);
        }
      }
    };
    auto one = [&](size_t t, const bool wrap) __attribute__((always_inline))
    {
      FD dla[G], dlb[G];
#pragma unroll
      for (int s = 0; s < G; ++s) { dla[s] = da[s][t]; dlb[s] = DIAG ? dla[s] : db[s][t]; }
      pool(dla, dlb, wrap);
    };
    unsigned c = c0;
    size_t t = t0;
    while (t < t1)
    {
      size_t run = maxc - c;                               // normal steps before the roll-over
      if (run > t1 - t) run = t1 - t;
      const size_t end = t + run;
      while (t < end)
      {
        if (t == next) flush(t);
        const size_t stop = next < end ? next : end;       // the window's samples before the roll-over
        if constexpr (KB > 1)
        {
          for (; t + KB <= stop; t += KB)                  // one s_load burst per channel and KB samples
          {
            FD dla[KB][G], dlb[KB][G];
#pragma unroll
            for (int s = 0; s < G; ++s)
#pragma unroll
              for (int u = 0; u < KB; ++u) { dla[u][s] = da[s][t + u]; dlb[u][s] = DIAG ? dla[u][s] : db[s][t + u]; }
#pragma unroll
            for (int u = 0; u < KB; ++u) pool(dla[u], dlb[u], false);
          }
        }
        for (; t < stop; ++t) one(t, false);
      }
      c += (unsigned)run;
      if (t < t1)
      {
        if (t == next) flush(t);
        one(t, true);
        ++t; c = 0;
      }
    }
    flush(t1);                                             // (t1 > t0: the last window of the chunk has samples)
  };
  if (diag) run(cov_flag<true>{});
  else run(cov_flag<false>{});

  if (last_chunk && writes)
  {
#pragma unroll
    for (int s = 0; s < G; ++s)
      if ((unsigned)s < na) store(sa[s], cha[s]);
  }
}

}  // namespace sdfthip
