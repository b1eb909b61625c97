// sdft_plan_launch.inc -- member functions of Plan<TD, FD> (included inside the class body by sdft_plan.hpp): the kernel
// launches.  A kernel is a template over the window, the slots per lane, the arithmetic flavour ...; the plan knows those at run
// time, so every launch is a small table from run-time values to one instantiation.  No decision is taken here beyond that
// table (which route and kernel form a call takes is decided in sdft_plan_logic.hpp: forward_route, inverse_route).

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
  // FD float, rows of a multiple of 128 bins, dense aligned output: the bin-pair kernel (sdft_forward_rows_f32.hpp; logic::ForwardRoute::rows_f32)
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
  void launch_forward_rows(const ForwardArgs<FD>& fa, unsigned blocks, unsigned threads, bool fused, bool rows_f32)
  {
    if constexpr (sizeof(FD) == 4)
    {
      if (rows_f32)
      {
        if (row_slots() == 1) launch_forward_rows_f32_s<1>(fa, blocks, threads, 0);
        else launch_forward_rows_f32_s<2>(fa, blocks, threads, 0);
        return;
      }
    }
    (void)rows_f32;
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
  void launch_forward_power(const ForwardArgs<FD>& fa, const PowerArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_power_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_power_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_power_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_power_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  void launch_forward_power_sum(const ForwardArgs<FD>& fa, const PowerSumArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_pooled_power_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_pooled_power_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_pooled_power_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_pooled_power_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  template <int HOLD> void launch_forward_power_peak_h(const ForwardArgs<FD>& fa, const PowerSumArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_power_peak_kernel<FD, BPL, WIN_HANN, HOLD>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_power_peak_kernel<FD, BPL, WIN_HAMMING, HOLD>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_power_peak_kernel<FD, BPL, WIN_BLACKMAN, HOLD>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_power_peak_kernel<FD, BPL, WIN_BOXCAR, HOLD>), gr, b, 0, stream, fa, g); break;
    }
  }
  void launch_forward_power_peak(const ForwardArgs<FD>& fa, const PowerSumArgs<FD>& g, unsigned blocks, int hold)
  {
    if (hold == logic::kHoldMin) launch_forward_power_peak_h<logic::kHoldMin>(fa, g, blocks); else launch_forward_power_peak_h<logic::kHoldMax>(fa, g, blocks);
  }
  template <int HOLD> void launch_forward_smooth_peak_h(const ForwardArgs<FD>& fa, const SmoothPeakArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_smooth_peak_kernel<FD, BPL, WIN_HANN, HOLD>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_smooth_peak_kernel<FD, BPL, WIN_HAMMING, HOLD>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_smooth_peak_kernel<FD, BPL, WIN_BLACKMAN, HOLD>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_smooth_peak_kernel<FD, BPL, WIN_BOXCAR, HOLD>), gr, b, 0, stream, fa, g); break;
    }
  }
  void launch_forward_smooth_peak(const ForwardArgs<FD>& fa, const SmoothPeakArgs<FD>& g, unsigned blocks, int hold)
  {
    if (hold == logic::kHoldMin) launch_forward_smooth_peak_h<logic::kHoldMin>(fa, g, blocks); else launch_forward_smooth_peak_h<logic::kHoldMax>(fa, g, blocks);
  }
  void launch_forward_power_smooth(const ForwardArgs<FD>& fa, const PowerSmoothArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_power_smooth_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_power_smooth_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_power_smooth_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_power_smooth_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  void launch_forward_cross_smooth(const ForwardArgs<FD>& fa, const CrossSmoothArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_cross_smooth_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_cross_smooth_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_cross_smooth_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_cross_smooth_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // their carry across chunks (chunks > 1) over `units` channels or pairs: one thread per (unit, number of the unit's row) scans the
  // chunks' end values in ascending order ...
  bool launch_smooth_scan(const PowerSmoothArgs<FD>& g, size_t n, long chunks, long len, long shift, size_t units)
  {
    const unsigned long long threads = (unsigned long long)units * g.nbins_out;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((smooth_scan_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, n, (unsigned)chunks, (unsigned)len, (unsigned)shift, (unsigned)units);
    return true;
  }
  // ... and one thread per (unit, kept row, number of the row) adds what a chunk c >= 1 left out of the row
  bool launch_smooth_fix(const PowerSmoothArgs<FD>& g, size_t rows, long chunks, long len, long shift, size_t units)
  {
    const unsigned long long threads = (unsigned long long)units * (unsigned long long)rows * g.nbins_out;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((smooth_fix_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, rows, (unsigned)chunks, (unsigned)len, (unsigned)shift, (unsigned)units);
    return true;
  }
  void launch_forward_filterbank(const ForwardArgs<FD>& fa, const FilterbankArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_filterbank_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_filterbank_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_filterbank_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_filterbank_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // the bands a tile boundary cuts, from their pieces in the workspace: one thread per (channel, row of the launch, split band)
  bool launch_filterbank_rows(const FilterbankArgs<FD>& g)
  {
    const unsigned long long threads = (unsigned long long)channels * (unsigned long long)g.ws_rows * g.nsplits;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((filterbank_rows_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, (unsigned)channels);
    return true;
  }
  // (g: the filterbank call's arguments, read with a pair where that call has a number: sdft_forward_band_peak.hpp)
  void launch_forward_band_peak(const ForwardArgs<FD>& fa, const FilterbankArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_band_peak_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_band_peak_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_band_peak_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_band_peak_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // the bands a tile boundary cuts, joined from their pieces' pairs by the rule: one thread per (channel, row of the launch, split band)
  bool launch_band_peak_rows(const FilterbankArgs<FD>& g)
  {
    const unsigned long long threads = (unsigned long long)channels * (unsigned long long)g.ws_rows * g.nsplits;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((band_peak_rows_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, (unsigned)channels);
    return true;
  }
  void launch_forward_cross_sum(const ForwardArgs<FD>& fa, const CrossSumArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_cross_sum_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_cross_sum_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_cross_sum_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_cross_sum_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // (g: the cross-spectrum call's arguments with the plan's channels in the pairs' place)
  void launch_forward_lag_sum(const ForwardArgs<FD>& fa, const CrossSumArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_lag_sum_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_lag_sum_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_lag_sum_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_lag_sum_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // (g: likewise; a row of nbins_out (s1, s2) pairs in the place of a row of complex sums)
  void launch_forward_power_moments(const ForwardArgs<FD>& fa, const CrossSumArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_power_moments_kernel<FD, BPL, WIN_HANN>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_power_moments_kernel<FD, BPL, WIN_HAMMING>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_power_moments_kernel<FD, BPL, WIN_BLACKMAN>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_power_moments_kernel<FD, BPL, WIN_BOXCAR>), gr, b, 0, stream, fa, g); break;
    }
  }
  // channels per group of a covariance call: the build's choice per FD type, or (test hook) a candidate of scripts/covariance_rates.py
  int array_group() const
  {
#ifdef SDFT_HIP_TEST_HOOKS
    if (opt_array_group == 1 || opt_array_group == 2 || opt_array_group == 4) return (int)opt_array_group;
#endif
    return cov_group<FD>::value;
  }
  template <int G> void launch_forward_covariance_g(const ForwardArgs<FD>& fa, const CovarianceArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_covariance_kernel<FD, BPL, WIN_HANN, G>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_covariance_kernel<FD, BPL, WIN_HAMMING, G>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_covariance_kernel<FD, BPL, WIN_BLACKMAN, G>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_covariance_kernel<FD, BPL, WIN_BOXCAR, G>), gr, b, 0, stream, fa, g); break;
    }
  }
  // (the items of g were built for array.group channels per group: the kernel's G must be that)
  bool launch_forward_covariance(const ForwardArgs<FD>& fa, const CovarianceArgs<FD>& g, unsigned blocks)
  {
    if (array.group == cov_group<FD>::value) { launch_forward_covariance_g<cov_group<FD>::value>(fa, g, blocks); return true; }
#ifdef SDFT_HIP_TEST_HOOKS
    switch (array.group)
    {
      case 1: launch_forward_covariance_g<1>(fa, g, blocks); return true;
      case 2: launch_forward_covariance_g<2>(fa, g, blocks); return true;
      case 4: launch_forward_covariance_g<4>(fa, g, blocks); return true;
      default: break;
    }
#endif
    set_error("sdft_hip_sdft_covariance_n", "no kernel for the array's group size");
    return false;
  }
  // channels per group and outputs per block of a mix call: the build's choice per FD type, or (test hooks) a candidate of
  // scripts/mix_rates.py
  int mix_group_size() const
  {
#ifdef SDFT_HIP_TEST_HOOKS
    if (opt_mix_group == 2 || opt_mix_group == 4 || opt_mix_group == 8) return (int)opt_mix_group;
#endif
    return mix_group<FD>::value;
  }
  int mix_block_size() const
  {
#ifdef SDFT_HIP_TEST_HOOKS
    if (opt_mix_block == 1 || opt_mix_block == 2 || opt_mix_block == 4) return (int)opt_mix_block;
#endif
    return mix_block<FD>::value;
  }
  template <int G, int O> void launch_forward_mix_go(const ForwardArgs<FD>& fa, const MixArgs<FD>& g, unsigned blocks)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 gr(blocks), b(kBlock);
    switch (window)
    {
      case WIN_HANN:     hipLaunchKernelGGL((forward_mix_kernel<FD, BPL, WIN_HANN, G, O>), gr, b, 0, stream, fa, g); break;
      case WIN_HAMMING:  hipLaunchKernelGGL((forward_mix_kernel<FD, BPL, WIN_HAMMING, G, O>), gr, b, 0, stream, fa, g); break;
      case WIN_BLACKMAN: hipLaunchKernelGGL((forward_mix_kernel<FD, BPL, WIN_BLACKMAN, G, O>), gr, b, 0, stream, fa, g); break;
      default:           hipLaunchKernelGGL((forward_mix_kernel<FD, BPL, WIN_BOXCAR, G, O>), gr, b, 0, stream, fa, g); break;
    }
  }
#ifdef SDFT_HIP_TEST_HOOKS
  template <int G> bool launch_forward_mix_g(const ForwardArgs<FD>& fa, const MixArgs<FD>& g, unsigned blocks)
  {
    switch (mix.block)
    {
      case 1: launch_forward_mix_go<G, 1>(fa, g, blocks); return true;
      case 2: launch_forward_mix_go<G, 2>(fa, g, blocks); return true;
      case 4: launch_forward_mix_go<G, 4>(fa, g, blocks); return true;
      default: return false;
    }
  }
#endif
  // (the items of g were built for mix.block outputs per block: the kernel's O must be that; G is the kernel's alone)
  bool launch_forward_mix(const ForwardArgs<FD>& fa, const MixArgs<FD>& g, unsigned blocks)
  {
    const int group = mix_group_size();
    if (group == mix_group<FD>::value && mix.block == mix_block<FD>::value)
    {
      launch_forward_mix_go<mix_group<FD>::value, mix_block<FD>::value>(fa, g, blocks);
      return true;
    }
#ifdef SDFT_HIP_TEST_HOOKS
    switch (group)
    {
      case 2: if (launch_forward_mix_g<2>(fa, g, blocks)) return true; break;
      case 4: if (launch_forward_mix_g<4>(fa, g, blocks)) return true; break;
      case 8: if (launch_forward_mix_g<8>(fa, g, blocks)) return true; break;
      default: break;
    }
#endif
    set_error("sdft_hip_sdft_mix_n", "no kernel for the mix's group and block size");
    return false;
  }
  // the rows of the windows a chunk boundary cuts, from their pieces in the workspace (chunks > 1); nch: the plan's channels, or the
  // pairs of a cross-spectrum or covariance call
  bool launch_power_sum_rows(const PowerSumArgs<FD>& g, size_t n, long chunks, long len, long shift, size_t nch)
  {
    const unsigned long long threads = (unsigned long long)nch * (unsigned long long)(chunks - 1) * g.nbins_out;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((pooled_power_rows_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, n, (unsigned)chunks, (unsigned)len, (unsigned)shift, (unsigned)nch);
    return true;
  }
  // likewise for the peak-hold call: the pieces combined by its rule
  bool launch_peak_rows(const PowerSumArgs<FD>& g, size_t n, long chunks, long len, long shift, size_t nch, int hold)
  {
    const unsigned long long threads = (unsigned long long)nch * (unsigned long long)(chunks - 1) * g.nbins_out;
    const unsigned long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_fits(blocks)) return false;
    hipLaunchKernelGGL((peak_rows_kernel<FD>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, g, n, (unsigned)chunks, (unsigned)len, (unsigned)shift, (unsigned)nch, hold);
    return true;
  }


  // rows in step (inverse_rows_body; where: logic::rows_in_step_ok)
  long last_inverse_nt = 0;                                  // the loads of the last synthesis launch were non-temporal ...
  long last_inverse_skip = 0;                                // ... but for its first last_inverse_skip rows
  long opt_inverse_step = 0;                                 // 1: always where it applies (tests, A/B); 0: a candidate of the tuner; -1: never
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
  // whole rows, ordered sum (inverse_rows_ordered_kernel; where: logic::rows_ordered_ok): rows of up to 8 KiB of terms
  long opt_inverse_ordered = 0;                              // 1: always where it applies (tests, A/B); 0: a candidate of the tuner, the static choice from 0.7 GB on; -1: never
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
  // every synthesis form: run-time form -> instantiation (rows_per_wave sizes the grid of the streaming forms).  false: the form
  // did not launch (the ordered form's LDS was refused, a host expression did not compile)
  template <bool LAT1, bool OPS> bool launch_inverse_form(int form, long rows_per_wave, const InverseArgs<TD, FD>& ia, size_t total_rows)
  {
    const size_t rw = (size_t)std::max(1L, rows_per_wave);
    const dim3 tiles((unsigned)std::min((total_rows + kWavesPerBlock - 1) / kWavesPerBlock, (size_t)256 * 8 * 4)), b(kBlock);
    const dim3 g((unsigned)std::max<size_t>(1, std::min<size_t>(((total_rows + rw - 1) / rw + kWavesPerBlock - 1) / kWavesPerBlock, (size_t)256 * 32)));
    switch (form)
    {
      case logic::F_TREE: hipLaunchKernelGGL((inverse_kernel<TD, FD, LAT1, OPS>), tiles, b, 0, stream, ia); return true;
      case logic::F_VERIFY:
        if constexpr (sizeof(TD) == 4 && sizeof(FD) == 8) hipLaunchKernelGGL((inverse_kernel<TD, FD, LAT1, OPS, true>), tiles, b, 0, stream, ia);
        return true;
      case logic::F_STEP: if constexpr (!OPS) launch_inverse_rows_in_step<LAT1>(ia, total_rows); return true;
      case logic::F_ORDERED: if constexpr (!OPS) return launch_inverse_rows_ordered<LAT1>(ia, total_rows); return true;
      case logic::F_ROW:
      {
        InverseArgs<TD, FD> ir = ia;
        ir.done = arm_flag((unsigned)total_rows);              // (the only form that signals its completion)
        if (OPS && ia.op.kind == OP_USER)
        {
          // the host's own statements inside the row synthesis of a hop: this instantiation, compiled at run time
          char name[160];
          snprintf(name, sizeof(name), "sdfthip::inverse_row_kernel<%s, %s, %s, true>", type_name<TD>(), type_name<FD>(), LAT1 ? "true" : "false");
          hipFunction_t fn = nullptr;
          if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) { rtc_failed = true; return false; }
          void* args[] = {&ir};
          if (hipModuleLaunchKernel(fn, (unsigned)total_rows, 1, 1, kWave, 1, 1, 0, stream, args, nullptr) != hipSuccess) { rtc_failed = true; return false; }
          return true;
        }
        hipLaunchKernelGGL((inverse_row_kernel<TD, FD, LAT1, OPS>), dim3((unsigned)total_rows), dim3(kWave), 0, stream, ir);
        return true;
      }
      case logic::F_32: if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 32, 1, false>), g, b, 0, stream, ia); return true;
      // (16 rows x 4 tiles in flight was measured in round 4 and lost to 4 x 8 below 64 Ki rows and to 16 x 1 above: scripts/inverse_ab.py)
      case logic::F_16: hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 16, 1, OPS>), g, b, 0, stream, ia); return true;
      case logic::F_16W: if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 16, 1, false, 2>), g, b, 0, stream, ia); return true;
      case logic::F_8: if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 8, 4, false>), g, b, 0, stream, ia); return true;
      case logic::F_8W: if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 8, 2, false, 2>), g, b, 0, stream, ia); return true;
      default: if constexpr (!OPS) hipLaunchKernelGGL((inverse_exact_kernel<TD, FD, LAT1, 4, 8, false>), g, b, 0, stream, ia); return true;   // F_4
    }
  }
  // The route (logic::inverse_route) decides the form, or the candidates the tuner picks from; this runs it and keeps the
  // tuner's books (a pair of events per timed candidate, reported once they have completed)
  template <bool LAT1, bool OPS> void launch_inverse(const InverseArgs<TD, FD>& ia, size_t total_rows)
  {
    flag_pending = false;                                    // only the one-wave-per-row form signals its completion
    last_inverse_nt = ia.nt; last_inverse_skip = (long)ia.nt_skip;
    logic::InverseQuery q;
    q.n = ia.n; q.channels = ia.channels; q.nbins = nbins; q.td_bytes = sizeof(TD); q.fd_bytes = sizeof(FD);
    q.in_stride = ia.in_stride; q.y_stride = ia.y_stride; q.in = reinterpret_cast<uintptr_t>(ia.in); q.row_pointers = ia.in_rows != nullptr;
    q.lat1 = LAT1; q.ops = OPS; q.nt = ia.nt != 0; q.nt_skip = ia.nt_skip; q.capacity4 = inverse_capacity[0]; q.capacity8 = inverse_capacity[1];
    q.exact = opt_exact_inverse; q.rows = opt_inverse_rows; q.step = opt_inverse_step; q.ordered = opt_inverse_ordered; q.tune = opt_inverse_tune;
    q.verify = opt_inverse_verify; q.nt_skip_mb = opt_inverse_nt_skip_mb;
    auto ordered_geometry = [&] { ordered_rows_geometry<FD> geo; return geo.make(nbins, ordered_lds()); };
    auto tune_events = [&] { return ensure_tune_events(); };
    auto capacity = [&](size_t& c4, size_t& c8)
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
      c4 = inverse_capacity[0]; c8 = inverse_capacity[1];
    };
    logic::InverseRoute r = logic::inverse_route(q, ordered_geometry, tune_events, capacity);
    while (!r.tuned)
    {
      if (!launch_inverse_form<LAT1, OPS>(r.form, r.rows_per_wave, ia, total_rows) && r.form == logic::F_ORDERED)
      {
        q.ordered_failed = true;                             // (its LDS was refused: the route without the static ordered form)
        r = logic::inverse_route(q, ordered_geometry, tune_events, capacity);
        continue;
      }
      last_inverse_form = logic::inverse_form_code(r.form);
      if (r.form == logic::F_STEP || r.form == logic::F_ORDERED) last_inverse_tuned = logic::inverse_tuned_code(r.form, false);
      return;
    }
    logic::TunerTable& table = inv_tunes[inv_after_write ? 1 : 0];
    const int tslot = table.find(total_rows, r.count);
    logic::FormTuner& tuner = table.slot[tslot];
    auto& tev = tune_evs[inv_after_write ? 1 : 0][tslot];
    for (int i = 0; i < r.count; ++i)
      if (tuner.inflight[i] && hipEventQuery(tev[i][1]) == hipSuccess)
      {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tev[i][0], tev[i][1]) != hipSuccess) ms = 0.f;
        tuner.report(i, ms);
      }
    (void)hipGetLastError();
    bool timed = false;
    const int pick = tuner.next(true, timed);
    const logic::InverseCandidate c = r.cand[pick];
    InverseArgs<TD, FD> it = ia;
    it.nt_skip = c.nt_skip;
    last_inverse_skip = (long)it.nt_skip;
    if (timed && hipEventRecord(tev[pick][0], stream) != hipSuccess) { (void)hipGetLastError(); timed = false; }
    last_inverse_form = logic::inverse_form_code(c.form);
    last_inverse_tuned = logic::inverse_tuned_code(c.form, tuner.chosen >= 0);
    (void)launch_inverse_form<LAT1, OPS>(c.form, logic::inverse_form_rows(c.form), it, total_rows);   // (not checked yet: ADVICE.md)
    if (timed) { if (hipEventRecord(tev[pick][1], stream) == hipSuccess) tuner.launched(pick); else (void)hipGetLastError(); }
  }
