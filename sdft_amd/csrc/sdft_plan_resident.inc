// sdft_plan_resident.inc -- member functions of Plan<TD, FD> (included inside the class body by sdft_plan.hpp): the host side of the resident
// hop kernel (sdft_resident.hpp; option "resident" = 1, off by default).  The reference driver's loop -- sdft_sdft_n + sdft_isdft_n per hop,
// synchronous, device pointers (/root/reference/test/test.c:69-83) -- then costs two doorbells instead of two launches.
//   * which calls: synchronous calls of one time chunk on a single-channel plan that owns its stream, device pointers on both sides, dense
//     matrices; the analysis as forward_hop would run it (two waves per tile, time parts), the synthesis as the wave-per-row form (<= 1024 rows);
//   * every other entry point retires the kernel first (bind() and synchronize() call resident_retire: a QUIT call, then the stream);
//   * the kernel leaves by itself after kResidentIdleUs without a call; a call that raced with that is told so by the exit word and the
//     kernel is started again; a call that is not served within kResidentBudgetMs makes the plan give the mode up (warning, ordinary launches).
  static constexpr unsigned kResidentIdleUs = 200;
  static constexpr unsigned kResidentBudgetMs = 200;
  static constexpr unsigned kResidentNoExit = 0xffffffffu;
  long opt_resident = 0;
  struct ResidentHost
  {
    unsigned* h = nullptr;       // pinned: line 0 = the call, line 1 word 0 = the exit word
    unsigned* d = nullptr;       // its device address
    bool alive = false;
    unsigned seq = 0;            // number of the last call submitted
    unsigned long long calls = 0, launches = 0, missed = 0;
  } res;
  DevBuf<unsigned> d_res;        // device: two copies of the call (32 words)

  bool resident_ready()
  {
    if (res.h) return true;
    if (!ensure_flag()) return false;
    if (!d_res.reserve(64)) return false;
    SDFT_TRY(hipMemsetAsync(d_res.p, 0, 64 * sizeof(unsigned), stream));
    unsigned* h = nullptr;
    if (hipHostMalloc((void**)&h, 128, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return false; }
    memset(h, 0, 128);
    unsigned* d = nullptr;
    if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return false; }
    res.h = h; res.d = d;
    return true;
  }
  void resident_release()
  {
    if (res.h) { (void)hipHostFree(res.h); res.h = nullptr; res.d = nullptr; }
    d_res.release();
  }

  template <int WIN> bool resident_launch_w(const ResidentArgs<TD, FD>& ra)
  {
    constexpr int BPL = sizeof(fdx) == 16 ? 1 : 2;
    const dim3 g(kResidentBlocks), b(2 * kWave);
    if (latency == 1) hipLaunchKernelGGL((resident_hop_kernel<TD, FD, BPL, WIN, true>), g, b, 0, stream, ra);
    else              hipLaunchKernelGGL((resident_hop_kernel<TD, FD, BPL, WIN, false>), g, b, 0, stream, ra);
    SDFT_TRY(hipGetLastError());
    return true;
  }
  bool resident_launch()
  {
    SDFT_TRY(hipSetDevice(device));
    if (!resident_ready()) return false;
    if (!pipe_join()) return false;
    ResidentArgs<TD, FD> ra;
    memset(&ra, 0, sizeof ra);
    // what forward_hop and inverse_device put into their arguments that does not change from call to call
    const long ntiles = tiles(), inter = interior_lanes();
    ra.ha.tw = d_tw.p; ra.ha.nbins = (unsigned)nbins; ra.ha.tiles = (unsigned)ntiles; ra.ha.interior_lanes = (unsigned)inter;
    ra.ha.total_waves = (unsigned long long)ntiles;
    ra.ha.wscale = (window == WIN_HANN) ? (FD)(tab.aweight * (FD)(0.25)) : tab.aweight;   // :371
    ra.ha.stamps = nullptr; ra.ha.parts = 1;
    ra.ia.syn = d_syn.p; ra.ia.nbins = (unsigned)nbins; ra.ia.channels = 1; ra.ia.sweight = tab.sweight;
    ra.ia.op = SpectralOp<FD>{}; ra.ia.op.kind = OP_IDENTITY; ra.ia.op.rows = 1;
    ra.ia.nt = 0; ra.ia.nt_skip = 0;
    for (int q = 0; q < 4; ++q) { ra.acc[q] = d_accs[q].p; ra.fid[q] = d_fids[q].p; ra.hist[q] = d_hist[q].p; }
    ra.host_call = res.d; ra.dev_call = d_res.p;
    ra.done_flag = d_done_flag; ra.done_count = d_done_count.p;
    ra.exit_word = res.d + 16;
    // (the device slots hold the QUIT the previous launch ended with -- numbered one beyond the last call it served: the calls of this
    // launch are numbered from beyond that, or its workgroups would take the stale QUIT for their first call)
    if (res.h[16] != kResidentNoExit && (int)(res.h[16] + 1u - res.seq) > 0) res.seq = res.h[16] + 1u;
    res.h[16] = kResidentNoExit;
    ra.first_seq = res.seq + 1u;
    ra.idle_ticks = kResidentIdleUs * 100u;                  // 100 MHz
    bool ok;
    switch (window)
    {
      case WIN_HANN:     ok = resident_launch_w<WIN_HANN>(ra); break;
      case WIN_HAMMING:  ok = resident_launch_w<WIN_HAMMING>(ra); break;
      case WIN_BLACKMAN: ok = resident_launch_w<WIN_BLACKMAN>(ra); break;
      default:           ok = resident_launch_w<WIN_BOXCAR>(ra); break;
    }
    if (!ok) return false;
    res.alive = true; ++res.launches;
    return true;
  }
  // QUIT, then the stream: what every entry point that is not a resident call does first
  bool resident_retire()
  {
    if (!res.alive) return true;
    res.alive = false;
    if (res.h[16] == kResidentNoExit)
    {
      ResidentCall c;
      memset(&c, 0, sizeof c);
      c.op = RES_QUIT;
      resident_ring(c);
    }
    SDFT_TRY(hipSetDevice(device));
    SDFT_TRY(hipStreamSynchronize(stream));
    return true;
  }
  // writes the call into the pinned line, the doorbell last
  void resident_ring(ResidentCall& c)
  {
    c.seq = ++res.seq;
    const unsigned* w = reinterpret_cast<const unsigned*>(&c);
    unsigned fold = 0;
    for (int i = 0; i < 14; ++i) fold ^= w[i];
    c.check = ~(c.seq ^ fold);
    volatile unsigned* line = res.h;
    for (int i = 0; i < 15; ++i) line[i] = w[i];
    std::atomic_thread_fence(std::memory_order_release);
    line[15] = w[15];
  }
  // submits a call and waits for its completion word; false: not served (the caller takes the ordinary route; the state is untouched)
  bool resident_call(ResidentCall& c)
  {
    using clock = std::chrono::steady_clock;
    for (int attempt = 0; attempt < 2; ++attempt)
    {
      // (a kernel that has left by its idle time-out says so in the exit word: no need to ring a doorbell nobody hears)
      if (res.alive && res.h[16] != kResidentNoExit)
      {
        res.alive = false;
        if (hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); opt_resident = 0; return false; }
      }
      if (!res.alive && !resident_launch()) { (void)hipGetLastError(); opt_resident = 0; return false; }
      c.flag_seq = ++flag_seq;
      resident_ring(c);
      volatile unsigned* f = h_done_flag;
      volatile unsigned* ex = res.h + 16;
      const clock::time_point t0 = clock::now();
      for (unsigned spins = 1;; ++spins)
      {
        if (*f == c.flag_seq) { ++res.calls; return true; }
        if ((spins & 63u) == 0)
        {
          if (*ex != kResidentNoExit)
          {
            // the kernel has left (idle time-out): after the stream has drained nothing can change any more
            res.alive = false;
            if (hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); opt_resident = 0; return false; }
            if (*f == c.flag_seq) { ++res.calls; return true; }           // served on its way out
            ++res.missed;
            break;                                                         // not served: start the kernel again and ring again
          }
          if (clock::now() - t0 > std::chrono::milliseconds(kResidentBudgetMs))
          {
            // nobody answers: give the mode up for this plan (the kernel's own time-outs end it; then the stream is clean)
            set_warning("resident_hop_kernel", "a call was not served in time; the plan goes back to one launch per call");
            opt_resident = 0;
            (void)resident_retire();
            return *f == c.flag_seq;
          }
        }
      }
    }
    return false;
  }

  // sdft_sdft_n as a resident call; false: not eligible or not served -- the caller goes on as if nothing had happened
  bool resident_analysis(size_t n, const TD* x, fdx* dfts)
  {
    if (async || profile != 0 || channels != 1 || !own_stream || stream_exposed || !opt_spin || !opt_hop_kernel || opt_chunk > 0) return false;
    if (nbins < 2 || n >= (size_t)logic::kHopSamples || n > (size_t)kHopMax) return false;
    if (!on_device(x) || !on_device(dfts)) return false;
    const size_t span = 2 * nbins;
    const long ntiles = tiles();
    if (ntiles > 2048) return false;
    const logic::HopParts hp = logic::hop_parts(n, (unsigned long long)ntiles, compute_units, opt_hop_parts, true);
    const unsigned long long blocks = (unsigned long long)ntiles * hp.parts;
    if (blocks > kResidentBlocks) return false;
    ResidentCall c;
    memset(&c, 0, sizeof c);
    c.x = reinterpret_cast<unsigned long long>(x); c.out = reinterpret_cast<unsigned long long>(dfts);
    c.n = (unsigned)n; c.cursor0 = (unsigned)cursor; c.parts = hp.parts; c.part_len = hp.part_len;
    c.slots = ((unsigned)st_cur & 3u) | (((unsigned)hist_cur & 3u) << 2);
    c.op = RES_ANALYSIS; c.blocks = (unsigned)blocks;
    if (!resident_call(c)) return false;
    calls.on_analysis(false);
    prev_out = logic::Range{0, 0};
    hist_cur ^= 1; st_cur ^= 1;
    last_kernel = 3; last_chunks = 1; last_chunk_len = (long)n; last_segments = 1; last_fused = 0; last_self = 0; last_prefix = 0; last_chain = 0;
    last_hop_pipe = 1; last_hop_parts = hp.parts; last_pipelined = 0;
    if (cursor + n >= span) fid_canonical = true;
    cursor = (cursor + n) % span;
    return true;
  }
  // sdft_sdft (sdft.h:562) as a resident call: the sample rides in the call's line, the row is device memory
  bool resident_analysis_sample(TD sample, fdx* dft)
  {
    if (profile != 0 || channels != 1 || !own_stream || stream_exposed || !opt_spin || !opt_hop_kernel || opt_chunk > 0) return false;
    if (nbins < 2 || !on_device(dft)) return false;
    const size_t span = 2 * nbins;
    const long ntiles = tiles();
    if (ntiles > (long)kResidentBlocks) return false;
    ResidentCall c;
    memset(&c, 0, sizeof c);
    c.out = reinterpret_cast<unsigned long long>(dft);
    memcpy(&c.y, &sample, sizeof(TD));
    c.n = 1; c.cursor0 = (unsigned)cursor; c.parts = 1; c.part_len = 1;
    c.slots = ((unsigned)st_cur & 3u) | (((unsigned)hist_cur & 3u) << 2);
    c.op = RES_ANALYSIS_SAMPLE; c.blocks = (unsigned)ntiles;
    if (!resident_call(c)) return false;
    calls.on_analysis(false);
    prev_out = logic::Range{0, 0};
    hist_cur ^= 1; st_cur ^= 1;
    last_kernel = 3; last_chunks = 1; last_chunk_len = 1; last_segments = 1; last_fused = 0; last_self = 0; last_prefix = 0; last_chain = 0;
    last_hop_pipe = 1; last_hop_parts = 1; last_pipelined = 0;
    if (cursor + 1 >= span) fid_canonical = true;
    cursor = (cursor + 1) % span;
    return true;
  }
  // sdft_isdft (sdft.h:635) as a resident call: the sample comes back through the plan's pinned scratch
  bool resident_synthesis_sample(const fdx* dft, TD* y)
  {
    if (!res.alive || !opt_pinned_io || !ensure_io()) return false;
    if (!resident_synthesis(1, dft, d_io, true)) return false;
    *y = *reinterpret_cast<volatile TD*>(h_io);
    return true;
  }
  // sdft_isdft_n as a resident call (y_is_device: the caller vouches for y -- the pinned scratch)
  bool resident_synthesis(size_t n, const fdx* dfts, TD* y, bool y_is_device = false)
  {
    if ((async && !y_is_device) || profile != 0 || channels != 1 || !own_stream || stream_exposed || !opt_spin) return false;
    if (nbins == 0 || n > 1024 || !opt_exact_inverse || opt_inverse_rows > 0) return false;
    if (!res.alive) return false;                            // (the analysis starts the kernel: a host that only synthesises keeps its launches)
    if (!on_device(dfts) || !(y_is_device || on_device(y))) return false;
    ResidentCall c;
    memset(&c, 0, sizeof c);
    c.out = reinterpret_cast<unsigned long long>(dfts); c.y = reinterpret_cast<unsigned long long>(y);
    c.n = (unsigned)n; c.op = RES_SYNTHESIS; c.blocks = (unsigned)n;
    if (!resident_call(c)) return false;
    inv_after_write = calls.prev_was_analysis;
    calls.on_synthesis_begin();
    calls.on_synthesis_launched();
    last_inverse_form = 1; last_inverse_pipelined = 0;
    return true;
  }
