// sdft_plan_launch.inc -- member functions of Plan<TD, FD> (included inside the class body by sdft_plan.hpp): the kernel
// launches.  A kernel is a template over the window, the slots per lane, the arithmetic flavour ...; the plan knows those at run
// time, so every launch is a small table from run-time values to one instantiation.  No decision is taken here beyond that
// table (which kernel FORM a call takes is decided in sdft_plan.hpp / sdft_plan_logic.hpp).

  template <int WIN, bool FUSED, int S>
  bool launch_forward_rows_self_ws(const ForwardArgs<FD>& fa, const SelfArgs<TD, FD>& sa, unsigned blocks, unsigned threads)
  {
    auto kern = forward_rows_kernel<FD, 1, WIN, FUSED, S, 0, true, TD, true>;
    const size_t lds = self_cells() * sizeof(fdx);
    static thread_local int raised_on = -1;                  // static + dynamic LDS beyond 64 KiB has to be asked for (per device)
    if (raised_on != device)
    {
      SDFT_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(96 * 1024)));
      raised_on = device;
    }
    const FuseArgs<TD, FD> none{};
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, stream, fa, none, sa);
    SDFT_TRY(hipGetLastError());
    return true;
  }
  template <bool FUSED>
  bool launch_forward_rows_self_t(const ForwardArgs<FD>& fa, const SelfArgs<TD, FD>& sa, unsigned blocks, unsigned threads)
  {
    const bool two = row_slots() != 1;
    switch (window)
    {
      case WIN_HANN:     return two ? launch_forward_rows_self_ws<WIN_HANN, FUSED, 2>(fa, sa, blocks, threads) : launch_forward_rows_self_ws<WIN_HANN, FUSED, 1>(fa, sa, blocks, threads);
      case WIN_HAMMING:  return two ? launch_forward_rows_self_ws<WIN_HAMMING, FUSED, 2>(fa, sa, blocks, threads) : launch_forward_rows_self_ws<WIN_HAMMING, FUSED, 1>(fa, sa, blocks, threads);
      case WIN_BLACKMAN: return two ? launch_forward_rows_self_ws<WIN_BLACKMAN, FUSED, 2>(fa, sa, blocks, threads) : launch_forward_rows_self_ws<WIN_BLACKMAN, FUSED, 1>(fa, sa, blocks, threads);
      default:           return two ? launch_forward_rows_self_ws<WIN_BOXCAR, FUSED, 2>(fa, sa, blocks, threads) : launch_forward_rows_self_ws<WIN_BOXCAR, FUSED, 1>(fa, sa, blocks, threads);
    }
  }
  bool launch_forward_rows_self(const ForwardArgs<FD>& fa, const SelfArgs<TD, FD>& sa, unsigned blocks, unsigned threads, bool fused)
  {
    // (FD double only: self_eligible; plain arithmetic only where the test hook "fused" = 0 can ask for it)
    if constexpr (sizeof(FD) == 8)
    {
#ifdef SDFT_HIP_TEST_HOOKS
      if (!fused) return launch_forward_rows_self_t<false>(fa, sa, blocks, threads);
#endif
      (void)fused;
      return launch_forward_rows_self_t<true>(fa, sa, blocks, threads);
    }
    else { (void)fused; set_error("forward_rows_kernel (self-carried)", "FD double only"); return false; }
  }


  template <bool ROWS, int WPB> void launch_hop_t(const HopArgs<TD, FD>& ha, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 g(blocks), b(kWave * WPB);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_hop_kernel<TD, FD, BPL, WIN_HANN, ROWS, WPB>), g, b, 0, stream, ha); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_hop_kernel<TD, FD, BPL, WIN_HAMMING, ROWS, WPB>), g, b, 0, stream, ha); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_hop_kernel<TD, FD, BPL, WIN_BLACKMAN, ROWS, WPB>), g, b, 0, stream, ha); break;
      default:           hipLaunchKernelGGL((forward_hop_kernel<TD, FD, BPL, WIN_BOXCAR, ROWS, WPB>), g, b, 0, stream, ha); break;
    }
  }

  template <bool ROWS> void launch_hop2_t(const HopArgs<TD, FD>& ha, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 g(blocks), b(2 * kWave);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_hop2_kernel<TD, FD, BPL, WIN_HANN, ROWS>), g, b, 0, stream, ha); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_hop2_kernel<TD, FD, BPL, WIN_HAMMING, ROWS>), g, b, 0, stream, ha); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_hop2_kernel<TD, FD, BPL, WIN_BLACKMAN, ROWS>), g, b, 0, stream, ha); break;
      default:           hipLaunchKernelGGL((forward_hop2_kernel<TD, FD, BPL, WIN_BOXCAR, ROWS>), g, b, 0, stream, ha); break;
    }
  }


  template <bool FUSED, int S> void launch_forward_rows_ts(const ForwardArgs<FD>& fa, unsigned blocks, unsigned threads)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 g(blocks), b(threads);
    const FuseArgs<TD, FD> none{};
    const SelfArgs<TD, FD> noself{};
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_rows_kernel<FD, BPL, WIN_HANN, FUSED, S, 0, true, TD>), g, b, 0, stream, fa, none, noself); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_rows_kernel<FD, BPL, WIN_HAMMING, FUSED, S, 0, true, TD>), g, b, 0, stream, fa, none, noself); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_rows_kernel<FD, BPL, WIN_BLACKMAN, FUSED, S, 0, true, TD>), g, b, 0, stream, fa, none, noself); break;
      default:           hipLaunchKernelGGL((forward_rows_kernel<FD, BPL, WIN_BOXCAR, FUSED, S, 0, true, TD>), g, b, 0, stream, fa, none, noself); break;
    }
  }
  template <bool FUSED> void launch_forward_rows_t(const ForwardArgs<FD>& fa, unsigned blocks, unsigned threads)
  {
    switch (row_slots())
    {
      case 1:  launch_forward_rows_ts<FUSED, 1>(fa, blocks, threads); break;
      default: launch_forward_rows_ts<FUSED, 2>(fa, blocks, threads); break;
    }
  }
  // FD float, rows of a multiple of 128 bins, dense aligned output: the bin-pair kernel (sdft_forward_rows_f32.hpp)
  long opt_rows_f32 = 1;
  long last_rows_f32 = 0;
  // (samples per lockstep group: 4; 2 measured slower -- 25.5 against 27.9 GB/s per CU, profiles/r04_kernels_beside_held_cus.txt)
  template <int S, int G = 4> void launch_forward_rows_f32_sg(const ForwardArgs<float>& fa, unsigned blocks, unsigned threads, size_t lds)
  {
    const dim3 g(blocks), b(threads);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_rows_f32_kernel<WIN_HANN, S, G>), g, b, lds, stream, fa); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_rows_f32_kernel<WIN_HAMMING, S, G>), g, b, lds, stream, fa); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_rows_f32_kernel<WIN_BLACKMAN, S, G>), g, b, lds, stream, fa); break;
      default:           hipLaunchKernelGGL((forward_rows_f32_kernel<WIN_BOXCAR, S, G>), g, b, lds, stream, fa); break;
    }
  }
  // (2 and 8 rows per group were measured in round 6 and lost or gained nothing in the call: profiles/r06_f32_rows_per_group.txt)
  template <int S> void launch_forward_rows_f32_s(const ForwardArgs<float>& fa, unsigned blocks, unsigned threads, size_t lds)
  {
    launch_forward_rows_f32_sg<S, 4>(fa, blocks, threads, lds);
  }
  // (rows of two slots, 2048 < N <= 4096, as two one-slot workgroups per row were built in round 5 -- same bits, 8-14 % slower,
  // profiles/r05_half_row_workgroups_*.txt -- and removed in round 6)
  void launch_forward_rows(const ForwardArgs<FD>& fa, unsigned blocks, unsigned threads, bool fused)
  {
    last_rows_f32 = 0;
    if constexpr (sizeof(FD) == 4)
    {
      if (opt_rows_f32 && nbins % (2 * kWave) == 0 && fa.vec_store && !fa.out_rows)
      {
        last_rows_f32 = 1;
        if (row_slots() == 1) launch_forward_rows_f32_s<1>(fa, blocks, threads, 0);
        else launch_forward_rows_f32_s<2>(fa, blocks, threads, 0);
        return;
      }
    }
    if constexpr (sizeof(FD) == 8) { if (fused) { launch_forward_rows_t<true>(fa, blocks, threads); return; } }
    launch_forward_rows_t<false>(fa, blocks, threads);
  }

  // fused analysis -> operation -> synthesis: the same kernel with SYN = 1 (tree sum over bins) or 2
  // (the reference's ascending order); the terms image lives in dynamic LDS
  size_t syn_lds(int syn) const
  {
    const size_t group = (size_t)syn_group((int)row_slots(), (int)bins_per_lane(), syn);   // samples per lockstep group (the kernel's G)
    const size_t padded = (size_t)row_waves() * (size_t)row_slots() * kWave * bins_per_lane();
    return (size_t)2 * group * (padded + 16 / sizeof(FD)) * sizeof(FD);          // double-buffered
  }
  template <int WIN, bool FUSED, int SYN, bool LAT1>
  bool launch_syn_w(const ForwardArgs<FD>& fa, const FuseArgs<TD, FD>& fz, unsigned blocks, unsigned threads)
  {
    return row_slots() == 1 ? launch_syn_ws<WIN, FUSED, SYN, LAT1, 1>(fa, fz, blocks, threads)
                            : launch_syn_ws<WIN, FUSED, SYN, LAT1, 2>(fa, fz, blocks, threads);
  }
  template <int WIN, bool FUSED, int SYN, bool LAT1, int S>
  bool launch_syn_ws(const ForwardArgs<FD>& fa, const FuseArgs<TD, FD>& fz, unsigned blocks, unsigned threads)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    auto kern = forward_rows_kernel<FD, BPL, WIN, FUSED, S, SYN, LAT1, TD>;
    static thread_local int raised_on = -1;                  // dynamic LDS beyond 64 KiB has to be asked for (per device)
    if (raised_on != device)
    {
      SDFT_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(140 * 1024)));
      raised_on = device;
    }
    if (fz.op.kind == OP_USER)
    {
      // the host's own operation: this instantiation, compiled at run time with its statements (sdft_common.hip)
      char name[256];
      snprintf(name, sizeof(name), "sdfthip::forward_rows_kernel<%s, %d, %d, %s, %d, %d, %s, %s, false>", type_name<FD>(), BPL, WIN,
               FUSED ? "true" : "false", S, SYN, LAT1 ? "true" : "false", type_name<TD>());
      hipFunction_t fn = nullptr;
      if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) return false;
      if (syn_lds(SYN) > (size_t)64 * 1024)
      {
        // a module function is not a host-side kernel symbol: hipFuncSetAttribute may refuse the handle (the launch below
        // then says so itself if the image does not fit); hipModule functions take what the launch asks for on this runtime
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(140 * 1024)) != hipSuccess)
          (void)hipGetLastError();
      }
      ForwardArgs<FD> a1 = fa; FuseArgs<TD, FD> f1 = fz; SelfArgs<TD, FD> s1{};
      void* args[] = {&a1, &f1, &s1};
      SDFT_TRY(hipModuleLaunchKernel(fn, blocks, 1, 1, threads, 1, 1, (unsigned)syn_lds(SYN), stream, args, nullptr));
      return true;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), syn_lds(SYN), stream, fa, fz, SelfArgs<TD, FD>{});
    SDFT_TRY(hipGetLastError());
    return true;
  }
  template <bool FUSED, int SYN, bool LAT1>
  bool launch_syn_t(const ForwardArgs<FD>& fa, const FuseArgs<TD, FD>& fz, unsigned blocks, unsigned threads)
  {
    switch (window)
    {
      case WIN_HANN:     return launch_syn_w<WIN_HANN, FUSED, SYN, LAT1>(fa, fz, blocks, threads);
      case WIN_HAMMING:  return launch_syn_w<WIN_HAMMING, FUSED, SYN, LAT1>(fa, fz, blocks, threads);
      case WIN_BLACKMAN: return launch_syn_w<WIN_BLACKMAN, FUSED, SYN, LAT1>(fa, fz, blocks, threads);
      default:           return launch_syn_w<WIN_BOXCAR, FUSED, SYN, LAT1>(fa, fz, blocks, threads);
    }
  }
  bool launch_syn(const ForwardArgs<FD>& fa, const FuseArgs<TD, FD>& fz, unsigned blocks, unsigned threads, bool fused, bool exact_order)
  {
    const bool lat1 = (latency == 1);                                           // :639 exact compare
    if (exact_order) return lat1 ? launch_syn_t<false, 2, true>(fa, fz, blocks, threads) : launch_syn_t<false, 2, false>(fa, fz, blocks, threads);
    if constexpr (sizeof(FD) == 8)
    {
      if (fused) return lat1 ? launch_syn_t<true, 1, true>(fa, fz, blocks, threads) : launch_syn_t<true, 1, false>(fa, fz, blocks, threads);
    }
    return lat1 ? launch_syn_t<false, 1, true>(fa, fz, blocks, threads) : launch_syn_t<false, 1, false>(fa, fz, blocks, threads);
  }


  static size_t process_tiles_bytes(unsigned threads) { return (size_t)(threads / kWave) * kProcGroup * kProcRow * sizeof(double); }
  template <int J, bool FUSED, bool HASB>
  bool launch_process_j(const ForwardArgs<FD>& fa, const ProcArgs<TD, FD>& pz, unsigned blocks, unsigned threads, const SelfArgs<TD, FD>* self)
  {
    const size_t tiles = process_tiles_bytes(threads);
    if (self)
    {
      if constexpr (sizeof(FD) == 8 && J <= 2)
      {
        // the chunk's differences in LDS beside the transpose tiles (at most 4 KiB: several workgroups share a CU)
        SelfArgs<TD, FD> sa = *self;
        sa.lds_deltas = fa.chunk_len <= 512 ? fa.chunk_len : 0u;
        auto kern = process_rows_kernel<TD, FD, J, FUSED, HASB, true>;
        static thread_local int raised_on = -1;              // dynamic LDS beyond 48 KiB has to be asked for (per device)
        if (raised_on != device)
        {
          SDFT_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(96 * 1024)));
          raised_on = device;
        }
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), tiles + sa.lds_deltas * sizeof(FD), stream, fa, pz, sa);
        return true;
      }
      set_error("sdft_hip_process_n", "internal: the self-carried form has one or two bins per lane");
      return false;
    }
    auto kern = process_rows_kernel<TD, FD, J, FUSED, HASB>;
    static thread_local int raised_on = -1;
    if (raised_on != device)
    {
      SDFT_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(96 * 1024)));
      raised_on = device;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), tiles, stream, fa, pz, SelfArgs<TD, FD>{});
    return true;
  }
  template <bool FUSED, bool HASB>
  bool launch_process_t(const ForwardArgs<FD>& fa, const ProcArgs<TD, FD>& pz, unsigned blocks, unsigned threads, long slots, const SelfArgs<TD, FD>* self)
  {
    if (slots <= 1) return launch_process_j<1, FUSED, HASB>(fa, pz, blocks, threads, self);
    if (slots == 2) return launch_process_j<2, FUSED, HASB>(fa, pz, blocks, threads, self);
    return launch_process_j<4, FUSED, HASB>(fa, pz, blocks, threads, self);
  }
  // waves of a fused-kernel workgroup and bins per lane (1, 2, 4).  FD double in the chunk-parallel path: two bins per lane
  // from 256 bins on -- the sum over bins (a transpose through LDS per wave and 8 samples) is paid per wave, the recurrence
  // per bin: n = 1e6, N = 1024: 0.485 -> 0.397 ms with 8 waves of 2 bins instead of 16 of 1
  // (four bins per lane where the call is long enough to fill the chip with such workgroups: 64 channels x 48000: 1.29 ->
  // 1.13 ms, n = 1e6: 0.397 -> 0.388 ms; n = 48000 alone: 0.038 -> 0.045 ms, so not there)
  void process_geometry(bool fused, long& waves, long& slots, size_t n = 0) const
  {
    const logic::ProcessGeometry g = logic::process_geometry(nbins, channels, n, fused, sizeof(FD), 0);
    waves = g.waves; slots = g.slots;
  }
  bool launch_process(const ForwardArgs<FD>& fa, const FuseArgs<TD, FD>& fz, unsigned blocks, bool fused, const SelfArgs<TD, FD>* self = nullptr)
  {
    ProcArgs<TD, FD> pz;
    pz.y = fz.y; pz.y_stride = fz.y_stride; pz.alpha = d_alpha.p; pz.beta = d_beta.p; pz.sweight = fz.sweight;
    pz.rows = coeff_rows; pz.hop = fz.op.hop;
    long waves, slots;
    process_geometry(fused, waves, slots, fa.n);
    const unsigned threads = (unsigned)(waves * kWave);
    const bool hasb = coeff_has_beta;
    bool ok;
    if constexpr (sizeof(FD) == 8)
    {
      if (fused)
      {
        ok = hasb ? launch_process_t<true, true>(fa, pz, blocks, threads, slots, self) : launch_process_t<true, false>(fa, pz, blocks, threads, slots, self);
        SDFT_TRY(hipGetLastError());
        return ok;
      }
    }
    ok = hasb ? launch_process_t<false, true>(fa, pz, blocks, threads, slots, self) : launch_process_t<false, false>(fa, pz, blocks, threads, slots, self);
    SDFT_TRY(hipGetLastError());
    return ok;
  }

  template <bool ROWS> void launch_forward_t(const ForwardArgs<FD>& fa, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 g(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_kernel<FD, BPL, WIN_HANN, ROWS>), g, b, 0, stream, fa); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_kernel<FD, BPL, WIN_HAMMING, ROWS>), g, b, 0, stream, fa); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_kernel<FD, BPL, WIN_BLACKMAN, ROWS>), g, b, 0, stream, fa); break;
      default:           hipLaunchKernelGGL((forward_kernel<FD, BPL, WIN_BOXCAR, ROWS>), g, b, 0, stream, fa); break;
    }
  }
  void launch_forward(const ForwardArgs<FD>& fa, unsigned blocks)
  {
    if (fa.out_rows) launch_forward_t<true>(fa, blocks); else launch_forward_t<false>(fa, blocks);
  }
  void launch_forward_every(const ForwardArgs<FD>& fa, const EveryGrid& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_every_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_every_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_every_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_every_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }


  // rows in step (inverse_rows_body): float samples from double bins at latency 1 (the term of a bin is +-re: one register per
  // bin in flight; the general term needs both halves and the kernel's three groups in flight no longer fit 64 registers),
  // dense rows of 64 ... 2048 bins; a form of the rounding-interval proof (option inverse_verify = 0 turns it off with the other one)
  long last_inverse_nt = 0;                                  // the loads of the last synthesis launch were non-temporal ...
  long last_inverse_skip = 0;                                // ... but for its first last_inverse_skip rows
  long opt_inverse_step = 0;                                 // 1: always where it applies (tests, A/B); 0: a candidate of the tuner; -1: never
  template <bool LAT1> bool rows_in_step_ok(const InverseArgs<TD, FD>& ia, size_t total_rows) const
  {
    return LAT1 && sizeof(TD) == 4 && sizeof(FD) == 8 && opt_inverse_verify && !ia.in_rows && nbins >= 64 && nbins <= 2048 && total_rows >= 64 && total_rows <= 0x7fffffffull * 4;
  }
  template <bool LAT1> void launch_inverse_rows_in_step(const InverseArgs<TD, FD>& ia, size_t total_rows)
  {
    if constexpr (LAT1 && sizeof(TD) == 4 && sizeof(FD) == 8)
    {
      const unsigned waves = (unsigned)(nbins <= 1024 ? (nbins + 63) / 64 : (nbins + 127) / 128);
      // about eight chunks per CU (two workgroups of 16 waves live on one): the chip's workgroups finish at different times
      size_t chunk = (total_rows + 2047) / 2048;
      chunk = std::max<size_t>(16, (chunk + 3) / 4 * 4);
      const size_t nchunks = (total_rows + chunk - 1) / chunk;
      if (nbins <= 1024) hipLaunchKernelGGL((inverse_rows1_kernel<TD, FD, LAT1>), dim3((unsigned)nchunks), dim3(waves * kWave), 0, stream, ia, (unsigned)chunk);
      else hipLaunchKernelGGL((inverse_rows2_kernel<TD, FD, LAT1>), dim3((unsigned)nchunks), dim3(waves * kWave), 0, stream, ia, (unsigned)chunk);
    }
  }
  // whole rows, ordered sum (inverse_rows_ordered_kernel): every type pair, any latency; rows of up to 8 KiB of terms in one run (one channel, or
  // channels without a gap between them), 16-byte loads
  long opt_inverse_ordered = 0;                              // 1: always where it applies (tests, A/B); 0: a candidate of the tuner, the static choice from 0.7 GB on; -1: never
  bool rows_ordered_ok(const InverseArgs<TD, FD>& ia, size_t total_rows) const
  {
    ordered_rows_geometry<FD> geo;
    const bool one_run = ia.channels == 1 || (ia.in_stride == ia.n * (size_t)nbins && ia.y_stride == ia.n);
    const bool loads_ok = (reinterpret_cast<uintptr_t>(ia.in) & 15) == 0 && (sizeof(cx<FD>) == 16 || nbins % 2 == 0);
    return !ia.in_rows && one_run && loads_ok && total_rows >= 64 && total_rows <= 0x7fffffffull && geo.make(nbins, ordered_lds());
  }
  // LDS of a workgroup: 140 KB hold 16 row slots of 8 KiB -- enough while a row has up to 1024 terms (the kernel is bound by HBM: 6.85 TB/s; with
  // more slots 6.75); rows of 1025 ... 2048 float terms are bound by the adding wave's chains, and 158 KB hold 18 slots in six groups:
  // 6.4 ... 6.6 TB/s against 5.6 ... 5.8 at 1e6 x 2048 (profiles/r06_synthesis_forms.txt)
  static constexpr size_t kOrderedLds = (size_t)140 * 1024, kOrderedLdsLong = (size_t)158 * 1024;
  bool ordered_long_rows() const { return nbins > 1024; }
  size_t ordered_lds() const { return ordered_long_rows() ? kOrderedLdsLong : kOrderedLds; }
  template <bool LAT1> bool launch_inverse_rows_ordered(const InverseArgs<TD, FD>& ia, size_t total_rows)
  {
    ordered_rows_geometry<FD> geo;
    if (!geo.make(nbins, ordered_lds())) return false;
    auto kern = inverse_rows_ordered_kernel<TD, FD, LAT1>;
    static thread_local int raised_on = -1;                  // dynamic LDS beyond 64 KiB has to be asked for (per device)
    if (raised_on != device)
    {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOrderedLdsLong) != hipSuccess) { (void)hipGetLastError(); return false; }
      raised_on = device;
    }
    // Chunks: a chunk's first rows wait for the loads and its last ones for the adding wave, so a chunk has 256 rows or more (n = 200 000 x 1024:
    // 6.6 TB/s with chunks of 196 ... 780 rows, 5.9 with 52); about sixteen chunks per CU where the matrix is long enough (n = 1e6: 512 ... 4096
    // chunks within 1 %; long rows, at the adding wave's pace: four); and never fewer chunks than CUs (n = 48 000: 256 chunks of 188 rows 6.1 TB/s,
    // 1500 chunks of 32 rows 4.7) -- scripts/inverse_forms_probe.hip
    size_t chunk = ordered_long_rows() ? (total_rows + 1023) / 1024 : (total_rows + 4095) / 4096;
    chunk = std::max<size_t>(chunk, 256);
    chunk = std::min<size_t>(chunk, std::max<size_t>((total_rows + 255) / 256, (size_t)8 * geo.G));
    chunk = (chunk + geo.G - 1) / geo.G * geo.G;
    const size_t nchunks = (total_rows + chunk - 1) / chunk;
    hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kWave * (ordered_rows_geometry<FD>::LOADERS + 1)), geo.lds_bytes, stream, ia, (unsigned)chunk, geo);
    return true;
  }
  template <bool LAT1, bool OPS> void launch_inverse(const InverseArgs<TD, FD>& ia, size_t total_rows)
  {
    size_t blocks = (total_rows + kWavesPerBlock - 1) / kWavesPerBlock;
    blocks = std::min(blocks, (size_t)256 * 8 * 4);
    flag_pending = false;                                    // only the row form below signals its completion
    last_inverse_nt = ia.nt; last_inverse_skip = (long)ia.nt_skip;
    // matrices from 6 GB on: the static choice too (n = 5e5 ... 1e6 x 1024, 64 x 48000 x 1024 / 2048, 250000 x 2048: +5 ... +10 % over
    // the best streaming form; 4 GB: a tie; below: the streaming forms, by up to 12 % -- profiles/r05_synthesis_rows_in_step.txt)
    const double matrix_bytes = (double)total_rows * (double)nbins * sizeof(cx<FD>);
    const bool step_static = opt_inverse_step >= 0 && rows_in_step_ok<LAT1>(ia, total_rows) && matrix_bytes >= 6.0e9;
    // (whole rows with the ordered sum: 6.85 TB/s at n = 1e6 x 1024 for every type pair -- rows in step 6.54, the tiles 5.8 ... 6.35;
    // profiles/r06_synthesis_forms.txt)
    const bool ordered_ok = !OPS && opt_exact_inverse && opt_inverse_rows <= 0 && opt_inverse_ordered >= 0 && rows_ordered_ok(ia, total_rows);
    const bool ordered_static = ordered_ok && matrix_bytes >= 7.0e8;      // (48 000 x 1024 double bins: 6.1 TB/s against 5.7 for the best of the tiles; 200 000: 6.65 against 6.2)
    if constexpr (!OPS)
    {
      const bool step_forced = opt_exact_inverse && opt_inverse_rows <= 0 && opt_inverse_step == 1 && opt_inverse_ordered != 1 && rows_in_step_ok<LAT1>(ia, total_rows);
      if (ordered_ok && !step_forced && (opt_inverse_ordered == 1 || (ordered_static && !opt_inverse_tune)))
      {
        if (launch_inverse_rows_ordered<LAT1>(ia, total_rows)) { last_inverse_form = 4; last_inverse_tuned = 7; return; }
      }
      if (opt_exact_inverse && opt_inverse_rows <= 0 && ((opt_inverse_step == 1 && rows_in_step_ok<LAT1>(ia, total_rows)) || (step_static && !opt_inverse_tune)))
      {
        launch_inverse_rows_in_step<LAT1>(ia, total_rows);
        last_inverse_form = 3; last_inverse_tuned = 6;
        return;
      }
    }
    if (!opt_exact_inverse)
    {
      hipLaunchKernelGGL((inverse_kernel<TD, FD, LAT1, OPS>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, ia);
      last_inverse_form = 0;
      return;
    }
    // the reference's summation order.  Measured (n=1e6, N=1024, f64): 32 rows per wave 2.75 ms, 16:
    // 2.82, 64: 3.6 (130 VGPRs); float bins and medium calls do best with 16; below 64 Ki rows a wave
    // with 16 rows and one tile of look-ahead is a chain of N/16 memory round trips (~70 us whatever
    // n is): 4 rows with an 8-deep ring (n = 12000: 33 us against 79, n = 48000: 153 against 178,
    // n = 131072: 397 against 355); short calls (a hop of 100 rows): one wave per row
    // float samples from double bins, medium calls: the tree-sum kernel with the rounding-interval test gives the same bits
    // without the chain of dependent additions (n = 4096: 22.5 -> 11.8 us, 48000: 145 -> 132 us, 200000: 585 -> 550 us;
    // from about half a million rows on the streaming kernel below is the faster one: 2.64 against 2.78 ms at n = 1e6)
    // Calls from 8 Ki rows on: the forms that stream at HBM speed differ by a few per cent either way from lease to lease -- 32 /
    // 16 / 8 / 4 rows per wave, 256- or 512-byte row segments, and (float samples from double bins) the tree sum with the
    // rounding-interval proof.  All give the same bits, so the plan measures them on the host's own calls (logic::FormTuner;
    // scripts/synthesis_forms_ab.py: n = 1e6 tree sum +5.5 %, 262144 x 1024 f64f64 16 rows +19 %, m = 4096 FD float 512-byte
    // segments +13 %; round 4's fixed switch points flipped winner five times between 16 k and 65 k rows).  Candidate 0 is the
    // static choice.  Forced forms (options inverse_rows / inverse_rpi / inverse_verify = 0) and operations: static.
    if constexpr (!OPS)
    {
      if (opt_inverse_tune && opt_inverse_rows <= 0 && total_rows >= 8192 && ensure_tune_events())
      {
        constexpr bool kProof = sizeof(TD) == 4 && sizeof(FD) == 8;
        enum { F_VERIFY = 0, F_32 = 1, F_16 = 2, F_16W = 3, F_8 = 4, F_4 = 5, F_STEP = 6, F_ORDERED = 7, F_8W = 8 };
        const bool verify0 = kProof && opt_inverse_verify && total_rows <= kInverseVerifyMax;
        const long rw0 = logic::inverse_rows_per_wave(total_rows, sizeof(FD), 0, inverse_capacity[0], inverse_capacity[1], false);
        const bool long_call = total_rows >= 65536;
        // candidates: up to kMax pairs (form, rows read first with ordinary loads).  The matrix streams past the caches (non-temporal loads) but for the
        // rows read first, which take ordinary loads: what an analysis left dirty in the Infinity Cache is slow to a non-temporal load.  1.5 GB of them
        // are the static choice from 6 GiB on and none below (logic::inverse_ordinary_rows); between 2 and 16 GiB which is better depends on the form
        // and on whether the host has just written the matrix (4.3 GB: TD = FD = double 1007 -> 835 us with them, f32f64 733 -> 779), so there every
        // form is tried both ways (profiles/r05_after_write_16gb.txt)
        int forms[logic::FormTuner::kMax]; size_t skips[logic::FormTuner::kMax]; int nf = 0;
        const bool both_loads = ia.nt && opt_inverse_nt_skip_mb < 0 && matrix_bytes >= 2.0 * 1073741824.0 && matrix_bytes < 16.0 * 1073741824.0;
        const size_t other_skip = ia.nt_skip ? 0 : logic::inverse_ordinary_rows((size_t)1 << 40, nbins * sizeof(cx<FD>), -1);
        auto add = [&](int f)
        {
          for (int i = 0; i < nf; ++i) if (forms[i] == f) return;
          if (nf < logic::FormTuner::kMax) { forms[nf] = f; skips[nf] = ia.nt_skip; ++nf; }
          if (both_loads && nf < logic::FormTuner::kMax) { forms[nf] = f; skips[nf] = other_skip; ++nf; }
        };
        add(ordered_static ? F_ORDERED : step_static ? F_STEP : verify0 ? F_VERIFY : (rw0 >= 32 ? F_32 : rw0 >= 16 ? F_16 : rw0 >= 8 ? F_8 : F_4));
        // (float samples from double bins: the two forms with the rounding-interval proof first)
        // (F_8W: 8 rows x 512 bytes, two tiles ahead -- the best of the tiles where rows are too long for the ordered form: 6.8 against 6.6 TB/s at
        // 500 000 x 2048 double; profiles/r06_synthesis_forms.txt)
        const int others_long[7] = {F_ORDERED, F_8W, F_STEP, F_VERIFY, F_16, F_32, F_16W}, others_medium[7] = {F_ORDERED, F_STEP, F_VERIFY, F_4, F_8, F_16, -1};
        int kinds = 1;
        for (int f : (long_call ? others_long : others_medium))
        {
          if (nf >= logic::FormTuner::kMax || kinds >= (both_loads ? 3 : 4)) break;
          if (f == forms[0]) continue;
          if (f < 0 || (f == F_ORDERED && !ordered_ok)) continue;
          if (f == F_8W && ordered_ok) continue;
          if (f == F_STEP && !(opt_inverse_step >= 0 && rows_in_step_ok<LAT1>(ia, total_rows))) continue;
          if (f == F_VERIFY && !(kProof && opt_inverse_verify)) continue;
          if (f == F_32 && sizeof(FD) != 8) continue;       // (64 registers of row segments: FD double only, as before)
          add(f); ++kinds;
        }
        logic::TunerTable& table = inv_tunes[inv_after_write ? 1 : 0];
        const int tslot = table.find(total_rows, nf);
        logic::FormTuner& tuner = table.slot[tslot];
        auto& tev = tune_evs[inv_after_write ? 1 : 0][tslot];
        for (int i = 0; i < nf; ++i)
          if (tuner.inflight[i] && hipEventQuery(tev[i][1]) == hipSuccess)
          {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, tev[i][0], tev[i][1]) != hipSuccess) ms = 0.f;
            tuner.report(i, ms);
          }
        (void)hipGetLastError();
        bool timed = false;
        const int pick = tuner.next(true, timed);
        const int form = forms[pick];
        InverseArgs<TD, FD> it = ia;
        it.nt_skip = skips[pick];
        last_inverse_skip = (long)it.nt_skip;
        if (timed && hipEventRecord(tev[pick][0], stream) != hipSuccess) { (void)hipGetLastError(); timed = false; }
        auto grid = [&](size_t rows_per_wave) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>(((total_rows + rows_per_wave - 1) / rows_per_wave + kWavesPerBlock - 1) / kWavesPerBlock, (size_t)256 * 32))); };
        last_inverse_form = form == F_VERIFY ? 2 : form == F_STEP ? 3 : form == F_ORDERED ? 4 : 1;
        last_inverse_tuned = 10 * (tuner.chosen >= 0 ? 1 : 0) + form;
        if constexpr (kProof) { if (form == F_VERIFY) hipLaunchKernelGGL((inverse_kernel<TD, FD, LAT1, false, true>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, it); }
        if (form == F_STEP) launch_inverse_rows_in_step<LAT1>(it, total_rows);
        if (form == F_ORDERED) (void)launch_inverse_rows_ordered<LAT1>(it, total_rows);     // (the attribute was granted when the form was found to apply ... or the launch fails and says so)
        if constexpr (sizeof(FD) == 8) { if (form == F_32) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 32, 1, false>), grid(32), dim3(kBlock), 0, stream, it); }
        if (form == F_16) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 16, 1, false>), grid(16), dim3(kBlock), 0, stream, it);
        else if (form == F_16W) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 16, 1, false, 2>), grid(16), dim3(kBlock), 0, stream, it);
        else if (form == F_8) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 8, 4, false>), grid(8), dim3(kBlock), 0, stream, it);
        else if (form == F_8W) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 8, 2, false, 2>), grid(8), dim3(kBlock), 0, stream, it);
        else if (form == F_4) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 4, 8, false>), grid(4), dim3(kBlock), 0, stream, it);
        if (timed) { if (hipEventRecord(tev[pick][1], stream) == hipSuccess) tuner.launched(pick); else (void)hipGetLastError(); }
        return;
      }
    }
    if constexpr (sizeof(TD) == 4 && sizeof(FD) == 8)
    {
      if (opt_inverse_verify && opt_inverse_rows <= 0 && total_rows > 1024 && total_rows <= kInverseVerifyMax)
      {
        hipLaunchKernelGGL((inverse_kernel<TD, FD, LAT1, OPS, true>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, ia);
        last_inverse_form = 2;
        return;
      }
    }
    last_inverse_form = 1;
    // (rows per wave: logic::inverse_rows_per_wave; the capacities of the 4-row and the 8-row form come from the occupancy API)
    if constexpr (!OPS)
    {
      if (opt_inverse_rows <= 0 && inverse_capacity[0] == 0 && total_rows > 1024 && total_rows < 65536)
      {
        int dev_cus = 0, b4 = 0, b8 = 0;
        if (hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4, inverse_exact_kernel<TD, FD, LAT1, 4, 8, false>, kBlock, 0) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&b8, inverse_exact_kernel<TD, FD, LAT1, 8, 4, false>, kBlock, 0) == hipSuccess)
        {
          inverse_capacity[0] = (size_t)std::max(1, b4) * dev_cus * kWavesPerBlock;
          inverse_capacity[1] = (size_t)std::max(1, b8) * dev_cus * kWavesPerBlock;
        }
        else { (void)hipGetLastError(); inverse_capacity[0] = inverse_capacity[1] = (size_t)-1; }
      }
    }
    const long rw = logic::inverse_rows_per_wave(total_rows, sizeof(FD), opt_inverse_rows, inverse_capacity[0], inverse_capacity[1], OPS);
    size_t eb = ((total_rows + rw - 1) / rw + kWavesPerBlock - 1) / kWavesPerBlock;
    eb = std::max<size_t>(1, std::min(eb, (size_t)256 * 32));
    const dim3 g((unsigned)eb), b(kBlock);
    if (rw == 1 && total_rows <= 0x7fffffffull)
    {
      InverseArgs<TD, FD> ir = ia;
      ir.done = arm_flag((unsigned)total_rows);
      if (OPS && ia.op.kind == OP_USER)
      {
        // the host's own statements inside the row synthesis of a hop: this instantiation, compiled at run time
        char name[160];
        snprintf(name, sizeof(name), "sdfthip::inverse_row_kernel<%s, %s, %s, true>", type_name<TD>(), type_name<FD>(), LAT1 ? "true" : "false");
        hipFunction_t fn = nullptr;
        if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) { rtc_failed = true; return; }
        void* args[] = {&ir};
        if (hipModuleLaunchKernel(fn, (unsigned)total_rows, 1, 1, kWave, 1, 1, 0, stream, args, nullptr) != hipSuccess) rtc_failed = true;
        return;
      }
      hipLaunchKernelGGL((inverse_row_kernel<TD, FD, LAT1, OPS>), dim3((unsigned)total_rows), dim3(kWave), 0, stream, ir);
    }
    else if (rw >= 32)
    {
      if constexpr (!OPS)
      {
        hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 32, 1, false>), g, b, 0, stream, ia);
      }
    }
    // (16 rows x 4 tiles in flight was measured in round 4 and lost to 4 x 8 below 64 Ki rows and to 16 x 1 above: scripts/inverse_ab.py)
    else if (rw >= 16)
    {
      hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 16, 1, OPS>), g, b, 0, stream, ia);
    }
    else if (rw >= 8)
    {
      if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 8, 4, false>), g, b, 0, stream, ia);
    }
    else
    {
      if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 4, 8, false>), g, b, 0, stream, ia);
    }
  }

