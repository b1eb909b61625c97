// sdft_plan_entry.inc -- member functions of Plan<TD, FD> (included inside the class body by sdft_plan.hpp): the entry points
// behind the C-ABI -- dense matrices or row-pointer tables, host or device pointers, single samples, the fused call, state
// access.  They run the routes sdft_plan_logic.hpp decides: host memory (logic::host_route), the fused call (logic::process_route).
// Citations are into /root/reference/c/src/sdft/sdft.h.

  // ---- host memory: the route of a call, and the one loop of the staged route ---------------------------------------
  // td: the samples side of the call, mat: its matrix side; td_map / mat_map receive the device-side address of a side the route
  // registered in place (whichever side the kernels write is registered writable)
  logic::HostRoute host_route(bool analysis, size_t n, const TD* td, bool td_device, bool by_value, const fdx* mat, bool mat_device, TD*& td_map, fdx*& mat_map)
  {
    logic::HostQuery q;
    q.analysis = analysis; q.samples_device = td_device; q.matrix_device = mat_device; q.by_value = by_value;
    q.samples_bytes = channels * n * sizeof(TD); q.matrix_bytes = matrix_bytes(n);
    q.pinned_io = opt_pinned_io; q.host_copy = io.opt_host_copy; q.host_direct = io.opt_host_direct;
    q.stage_bytes = stage_bytes; q.n = n; q.row_bytes = channels * nbins * sizeof(fdx);
    return logic::host_route(q, [&] { return ensure_io(); },
                             [&] { return (mat_map = static_cast<fdx*>(map_host(mat, q.matrix_bytes, analysis))) != nullptr; },
                             [&] { return (td_map = static_cast<TD*>(map_host(td, q.samples_bytes, !analysis))) != nullptr; },
                             [&] { return io.ensure_pin(); }, [&] { return io.pin_idle(); });
  }

  // A call in time segments of at most `seg` samples: a side that is host memory goes through device scratch (copied in before
  // the segment runs, out after it), a side that is device memory is used where it is.  run(Segment&) does the segment's device
  // call on s.td / s.mat; an analysis that keeps fewer rows than samples (sdft_every_n, sdft_power_n) sets s.row0 / s.rows, the
  // rows copied out.  The matrix side is rows of row_bytes bytes per channel -- complex bins (fdx rows of N) or the real numbers of
  // a band (sdft_power_n) --; s.mat_rows is the number of rows from one channel to the next in s.mat.
  struct StagedCall
  {
    bool analysis; TD* td; bool td_host; void* mat; bool mat_host;
    size_t mat_rows, seg_rows;                               // matrix rows of the whole call; of one segment, at most
    size_t row_bytes;                                        // of one channel's row
  };
  struct Segment
  {
    size_t t, m; TD* td; size_t td_stride; void* mat; size_t mat_rows, row0, rows;
    fdx* bins() const { return static_cast<fdx*>(mat); }     // the matrix side as rows of complex bins
  };
  size_t bins_row_bytes() const { return nbins * sizeof(fdx); }
  template <class Run>
  bool staged_segments(size_t n, size_t seg, const StagedCall& c, Run&& run)
  {
    const size_t rb = c.row_bytes;
    char* const mat = static_cast<char*>(c.mat);
    if (c.td_host && !d_stage_td.reserve(channels * seg)) return false;
    if (c.mat_host && !d_stage_fdx.reserve((channels * c.seg_rows * rb + sizeof(fdx) - 1) / sizeof(fdx))) return false;
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      Segment s{t, m, c.td_host ? d_stage_td.p : c.td + t, c.td_host ? m : n,
                c.mat_host ? static_cast<void*>(d_stage_fdx.p) : (mat ? static_cast<void*>(mat + t * rb) : nullptr), c.mat_host ? m : c.mat_rows, t, m};
      if (c.analysis && c.td_host && !copy2d(s.td, m * sizeof(TD), c.td + t, n * sizeof(TD), m * sizeof(TD), hipMemcpyHostToDevice)) return false;
      if (!c.analysis && c.mat_host && !copy2d(s.mat, m * rb, mat + t * rb, n * rb, m * rb, hipMemcpyHostToDevice)) return false;
      if (!run(s)) return false;
      if (c.analysis && c.mat_host && s.rows &&
          !copy2d(mat + s.row0 * rb, c.mat_rows * rb, s.mat, s.rows * rb, s.rows * rb, hipMemcpyDeviceToHost)) return false;
      if (!c.analysis && c.td_host && !copy2d(c.td + t, n * sizeof(TD), s.td, m * sizeof(TD), m * sizeof(TD), hipMemcpyDeviceToHost)) return false;
      SDFT_TRY(hipStreamSynchronize(stream));                // scratch buffers are reused; host memory is complete on return
    }
    return synchronize();
  }

  // host samples through device scratch (one small copy); nullptr: failed
  const TD* staged_samples(const TD* x, size_t count)
  {
    if (!d_stage_td.reserve(count) || !to_device(d_stage_td.p, x, count * sizeof(TD))) return nullptr;
    return d_stage_td.p;
  }

  // ---- public entry points: dense matrices, host or device pointers ---------------------------
  // x: [channels][n], dfts: [channels][n][N]
  // x_class: -1 = classify x, 0 = x is host memory whatever option "pointers" says (by-value sample)
  bool sdft_n(size_t n, const TD* x, fdx* dfts, int x_class = -1)
  {
    if (n == 0 || nbins == 0) return true;
    if (opt_resident && x_class < 0 && resident_analysis(n, x, dfts)) return true;      // (no runtime call at all: a doorbell and a completion word)
    if (opt_resident && x_class == 0 && n == 1 && resident_analysis_sample(x[0], dfts)) return true;    // sdft_sdft: the sample rides in the call
    if (!bind()) return false;
    const bool xd = x_class < 0 ? on_device(x) : x_class != 0;
    const bool od = on_device(dfts);
    TD* x_map = nullptr; fdx* o_map = nullptr;
    const logic::HostRoute r = host_route(true, n, x, xd, x_class == 0, dfts, od, x_map, o_map);
    if (r.refused) return copy_failed();
    if (r.route == logic::HR_STAGED)
      return staged_segments(n, r.seg, StagedCall{true, const_cast<TD*>(x), !xd, dfts, !od, n, r.seg, bins_row_bytes()},
                             [&](Segment& s) { return forward_device(s.m, s.td, s.td_stride, s.bins(), s.mat_rows * nbins, nullptr); });
    // one launch on the whole call: the samples and the matrix as the kernels see them
    const size_t xbytes = channels * n * sizeof(TD), obytes = matrix_bytes(n);
    const bool direct = r.route == logic::HR_DIRECT;
    const TD* xs = r.samples == logic::HS_MAPPED ? x_map : x;
    if (r.samples == logic::HS_IO) { memcpy(h_io, x, xbytes); xs = d_io; }
    if (r.samples == logic::HS_STAGE_TD && !(xs = staged_samples(x, channels * n))) return false;
    fdx* out = direct ? reinterpret_cast<fdx*>(io.d_pin) : (od ? dfts : o_map);
    // (the flags hold until the function returns; only the launches read them -- arm_flag, hop_parts, the pipe tests -- not finish)
    Scoped<bool> sync(async, async && !r.synchronous), flag(flag_wanted, r.flag_wanted), pipe(pipe_allowed, r.pipe_allowed);
    if (direct) ++io.pin_copies;
    const double t0 = direct ? HostIo::now_us() : 0.0;
    if (!forward_device(n, xs, n, out, n * nbins, nullptr)) return false;
    if (!(r.end == logic::HE_FINISH ? finish(obytes) : finish_mapped(obytes))) return false;
    if (direct)
    {
      // the kernels wrote the plan's pinned pieces: the host copies the matrix out
      const double t1 = HostIo::now_us();
      io.copy_bytes(dfts, io.h_pin, obytes);
      io.pin_us_device += t1 - t0; io.pin_us_memcpy += HostIo::now_us() - t1;
    }
    return true;
  }

  // ---- grid analysis calls: sdft_every_n and its thirteen siblings ---------------------------------------------------------------
  // What the fourteen share.  The stream state after a call is the one sdft_n leaves on the same samples.  A call is never resident,
  // pipelined or fused: whatever is in flight is retired / joined first, then one forward call on the plan's stream with the
  // call's own kernel (ForwardCall).  `rows` receives the row count.  Device samples and a device output take that one call; host
  // memory goes through device scratch in time segments of at most logic::grid_segment samples, each segment a call of its own
  // under the streaming contract, with its own first.
  // The every-grid calls (every, power, power_smooth, cross_smooth, filterbank, band_peak, mix) keep the rows of the samples first, first + every, ... < n; a segment
  // keeps the rows of the grid that fall into it.  The pooled calls (power_sum, power_peak, smooth_peak, power_moments, cross_sum, lag_sum, covariance) write
  // one row per window the grid cuts the call into (logic::power_sum_window), row 0 the head window [0, first) when first > 0; a
  // segment that starts inside a window has a head row of its own, which is kept apart (the call's head buffer) and joined into
  // the row the segment before it ended with -- on the host for a host buffer, by a small kernel for a device buffer.
  // The output is dense [units][rows][unit_row] numbers: the units are the plan's channels, or the pairs / outputs a call has
  // installed.  Rows on their way to a host buffer go through staged_segments' own scratch and copy (per channel), or -- where
  // the units are not the channels, or the kernel re-reads what it wrote -- through a stage buffer of the call's and out unit by unit.

  // one forward call of a grid analysis -- the whole call, or a segment of it on device scratch -- with its grid
  struct GridPiece { size_t m; const TD* td; size_t td_stride; EveryGrid grid; };

  // The argument checks of a grid call, in the order a host sees them win: the grid, the band (has_band: the call takes one), the
  // call's own (refused: its message, or nullptr), the output.  pooled: the rows are windows, which the call "writes".
  bool grid_args(const char* fn, size_t n, size_t every, size_t first, bool has_band, size_t bin0, size_t nbins_out, const char* refused,
                 bool pooled, const void* out, const char* out_name, size_t& rows)
  {
    rows = 0;
    if (every == 0) { set_error(fn, "every must be at least 1"); return false; }
    if (has_band && nbins_out == 0) { set_error(fn, "nbins must be at least 1"); return false; }
    if (has_band && !logic::power_band_ok(nbins, bin0, nbins_out)) { set_error(fn, "the band bin0 ... bin0 + nbins - 1 does not lie within the plan's bins"); return false; }
    if (refused) { set_error(fn, refused); return false; }
    rows = pooled ? logic::power_sum_rows(n, every, first) : logic::every_rows(n, every, first);
    if (rows > 0 && !out) { set_error(fn, (std::string(out_name) + " is NULL but the call " + (pooled ? "writes" : "keeps") + " rows").c_str()); return false; }
    return true;
  }
  static bool grid_ready() { return true; }                  // (a call with nothing to re-upload)

  // The every-grid calls, after grid_args.  ready(): what the call prepares once the plan is bound and joined (tables a test hook
  // invalidated).  launch(piece, at, at_rows): builds the call's arguments for the rows at `at` ([units][at_rows][unit_row] of T)
  // and runs forward_device.  stage: the call's own stage buffer (see above), nullptr: staged_segments' (units == channels).
  template <class T, class Ready, class Launch>
  bool every_grid_call(size_t n, const TD* x, size_t every, size_t first, T* out, size_t rows, size_t units, size_t unit_row,
                       Ready&& ready, Launch&& launch, DevBuf<T>* stage = nullptr)
  {
    if (n == 0) return true;
    if (!bind() || !pipe_join() || !ready()) return false;
    if (every > n) every = n;                                // (the same grid: at most one row; keeps first + k * every in range)
    const bool xd = on_device(x);
    const bool od = rows == 0 || on_device(out);
    const size_t row_bytes = units * unit_row * sizeof(T);
    if (xd && od) return launch(GridPiece{n, x, n, {every, first}}, out, rows) && finish(rows * row_bytes);
    const size_t seg = logic::grid_segment(n, every, first, row_bytes, channels * sizeof(TD), stage_bytes, xd, od, false);
    const size_t seg_rows_max = (seg + every - 1) / every;
    if (stage && !od && !stage->reserve(units * seg_rows_max * unit_row)) return false;
    const StagedCall c{true, const_cast<TD*>(x), !xd, stage ? nullptr : out, !stage && !od, rows, seg_rows_max, unit_row * sizeof(T)};
    return staged_segments(n, seg, c, [&](Segment& s) {
      const size_t f = logic::every_first_from(s.t, every, first);
      const size_t kept = logic::every_rows(s.m, every, f);
      const size_t r0 = kept ? (s.t + f - first) / every : 0; // the segment's first row in the call's grid
      s.row0 = r0; s.rows = stage ? 0 : kept;                // (a call with a stage buffer leaves staged_segments nothing to copy)
      T* const at = od ? (kept ? out + r0 * unit_row : nullptr) : stage ? stage->p : static_cast<T*>(s.mat);
      if (!launch(GridPiece{s.m, s.td, s.td_stride, {every, f}}, at, od ? rows : kept)) return false;
      for (size_t u = 0; u < units && stage && !od && kept; ++u)
        if (!to_host(out + (u * rows + r0) * unit_row, stage->p + u * kept * unit_row, kept * unit_row * sizeof(T))) return false;
      return true;
    });
  }

  // The pooled calls, after grid_args; ready() as above.  launch(piece, row0, row0_stride, rest, rest_stride): builds the call's
  // arguments for a first row at row0 and the rows after it at rest, and runs forward_device.  head: the call's head buffer.
  // hold: how a head row joins the row it completes -- kJoinAdd: it is added (pooled_power_add_kernel, + on the host); 0 / 1: the
  // peak-hold call's rule (peak_join_kernel, logic::peak_hold), which is associative and commutative: there, how the segments cut
  // a window does not show in the bits.
  static constexpr int kJoinAdd = -1;
  template <class Ready, class Launch>
  bool pooled_grid_call(size_t n, const TD* x, size_t every, size_t first, FD* out, size_t rows, size_t units, size_t unit_row,
                        DevBuf<FD>& head, DevBuf<FD>* stage, int hold, Ready&& ready, Launch&& launch)
  {
    if (n == 0) return true;
    if (!bind() || !pipe_join() || !ready()) return false;
    if (every > n) every = n;                                // (the same windows; keeps first + k * every in range)
    const bool xd = on_device(x);
    const bool od = on_device(out);
    const size_t row_bytes = units * unit_row * sizeof(FD);
    const size_t stride = logic::power_channel_stride(rows, unit_row);
    if (xd && od) return launch(GridPiece{n, x, n, {every, first}}, out, stride, out + unit_row, stride) && finish(rows * row_bytes);
    const size_t seg = logic::grid_segment(n, every, first, row_bytes, channels * sizeof(TD), stage_bytes, xd, od, true);
    const size_t seg_rows_max = (seg + every - 1) / every + 1;
    if (stage && !od && !stage->reserve(units * seg_rows_max * unit_row)) return false;
    std::vector<FD> head_host;                               // host buffers: a segment's head rows on their way to the rows they complete
    const StagedCall c{true, const_cast<TD*>(x), !xd, stage ? nullptr : out, !stage && !od, rows, seg_rows_max, unit_row * sizeof(FD)};
    return staged_segments(n, seg, c, [&](Segment& s) {
      const size_t f = logic::every_first_from(s.t, every, first);
      const logic::PowerSumWindow w0 = logic::power_sum_window(s.t, n, every, first);      // of the segment's row 0 in the call
      const bool joins = w0.begin < s.t;                     // row 0 is a head: it completes row w0.row of the call
      const size_t kept = logic::power_sum_rows(s.m, every, f) - (joins ? 1 : 0);
      if (joins && !head.reserve(units * unit_row)) return false;
      const size_t r0 = w0.row + (joins ? 1 : 0);            // the segment's first row of its own
      s.row0 = r0; s.rows = stage ? 0 : kept;                // (a call with a stage buffer leaves staged_segments nothing to copy)
      FD* const at = od ? out + r0 * unit_row : stage ? stage->p : static_cast<FD*>(s.mat);      // scratch: [units][kept][unit_row]
      const size_t at_stride = od ? stride : kept * unit_row;
      const GridPiece piece{s.m, s.td, s.td_stride, {every, f}};
      if (!(joins ? launch(piece, head.p, unit_row, at, at_stride) : launch(piece, at, at_stride, at + unit_row, at_stride))) return false;
      FD* const joined = out + w0.row * unit_row;            // (of unit 0) the row a head completes
      if (od)
      {
        if (!joins) return true;
        const unsigned long long threads = (unsigned long long)units * unit_row;
        const dim3 blocks((unsigned)((threads + kBlock - 1) / kBlock));
        if (hold == kJoinAdd) hipLaunchKernelGGL((pooled_power_add_kernel<FD>), blocks, dim3(kBlock), 0, stream, joined, stride, head.p, (unsigned)unit_row, (unsigned)units);
        else hipLaunchKernelGGL((peak_join_kernel<FD>), blocks, dim3(kBlock), 0, stream, joined, stride, head.p, (unsigned)unit_row, (unsigned)units, hold);
        SDFT_TRY(hipGetLastError());
        return true;
      }
      for (size_t u = 0; u < units && stage && kept; ++u)
        if (!to_host(out + u * stride + r0 * unit_row, stage->p + u * kept * unit_row, kept * unit_row * sizeof(FD))) return false;
      if (!joins) return true;
      head_host.resize(units * unit_row);
      if (!to_host(head_host.data(), head.p, head_host.size() * sizeof(FD))) return false;
      SDFT_TRY(hipStreamSynchronize(stream));
      for (size_t u = 0; u < units; ++u)
        for (size_t k = 0; k < unit_row; ++k)
        {
          FD& to = joined[u * stride + k];
          to = hold == kJoinAdd ? to + head_host[u * unit_row + k] : logic::peak_hold(to, head_host[u * unit_row + k], hold);
        }
      return true;
    });
  }

  // decimated analysis (sdft_hip_sdft_every_n): the rows sdft_n would write on the grid, dense [channels][rows][N]
  // (forward_every_kernel); the full grid is the analysis itself
  bool sdft_every_n(size_t n, const TD* x, size_t every, size_t first, fdx* dfts, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_every_n", n, every, first, false, 0, 0, nullptr, false, dfts, "dfts", rows)) return false;
    if (n == 0 || nbins == 0) return true;
    if (every == 1 && first == 0) return sdft_n(n, x, dfts);      // every row: the analysis itself
    return every_grid_call(n, x, every, first, dfts, rows, channels, nbins, grid_ready, [&](const GridPiece& p, fdx* at, size_t at_rows) {
      return forward_device(p.m, p.td, p.td_stride, at, at_rows * nbins, nullptr, ForwardCall::decimated(p.grid));
    });
  }

  // power-spectrogram analysis (sdft_hip_sdft_power_n): re^2 + im^2 of the bins [bin0, bin0 + nbins_out) of the rows of the grid,
  // dense [channels][rows][nbins_out] real numbers (bins outside the band step all the same) -- forward_power_kernel, for the
  // full grid and the full band too
  bool sdft_power_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* power, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_power_n", n, every, first, true, bin0, nbins_out, nullptr, false, power, "power", rows)) return false;
    return every_grid_call(n, x, every, first, power, rows, channels, nbins_out, grid_ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
      const PowerArgs<FD> g{at, logic::power_channel_stride(at_rows, nbins_out), p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::band_power(g));
    });
  }

  // smoothed power analysis (sdft_hip_sdft_power_smooth_n): s[t] = fl(fl(a * s[t - 1]) + fl(b * p[t])) of sdft_power_n's every == 1
  // powers, advanced at every sample and kept on the grid, dense [channels][rows][nbins_out] real numbers --
  // forward_power_smooth_kernel, then, in a call of more than one chunk, smooth_scan_kernel and smooth_fix_kernel.  sdft_power_n's
  // path with one addition: s travels from the caller's state [channels][nbins_out] (host or device memory; nullptr: from zero,
  // and the end value is dropped) through the two halves of d_smooth_state -- a launch reads one and writes the other, the next
  // segment of a call on host memory goes on from there -- and back to the caller once the whole call has succeeded.  A call in
  // several segments reports their number as "last_segments".
  bool sdft_power_smooth_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, double decay, FD* state, FD* smooth,
                           size_t& rows)
  {
    const char* const refused = logic::power_smooth_decay_ok<FD>(decay) ? nullptr : "decay must be at least 0 and less than 1 after rounding to sdft_fd_t";
    if (!grid_args("sdft_hip_sdft_power_smooth_n", n, every, first, true, bin0, nbins_out, refused, false, smooth, "smooth", rows)) return false;
    if (n == 0 || nbins == 0) return true;
    const FD a = (FD)decay, b = (FD)1 - a;
    const size_t count = channels * nbins_out;
    bool state_device = false;
    int cur = 0;                                             // the half of d_smooth_state that holds s
    long pieces = 0;                                         // forward calls: more than one when host memory goes in segments
    auto ready = [&] {
      if (!d_smooth_state.reserve(2 * count)) return false;
      state_device = state && on_device(state);
      if (!state) SDFT_TRY(hipMemsetAsync(d_smooth_state.p, 0, count * sizeof(FD), stream));
      else if (state_device) SDFT_TRY(hipMemcpyAsync(d_smooth_state.p, state, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
      else if (!to_device(d_smooth_state.p, state, count * sizeof(FD))) return false;
      return true;
    };
    if (!every_grid_call(n, x, every, first, smooth, rows, channels, nbins_out, ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
          const PowerSmoothArgs<FD> g{at, logic::power_channel_stride(at_rows, nbins_out), d_smooth_state.p + cur * count, d_smooth_state.p + (cur ^ 1) * count,
                                      nullptr, nullptr, a, b, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
          if (!forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::power_smooth(g))) return false;
          cur ^= 1; ++pieces;
          return true;
        })) return false;
    if (pieces > 1) last_segments = pieces;                  // ("last_segments": the call went in that many time segments, each a call with its own carries)
    if (!state) return true;
    if (!state_device) return to_host(state, d_smooth_state.p + cur * count, count * sizeof(FD));
    SDFT_TRY(hipMemcpyAsync(state, d_smooth_state.p + cur * count, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
    return async || synchronize();
  }

  // ---- filterbank analysis ---------------------------------------------------------------------------------------------
  // the decomposition of a filterbank for the plan's tiles and its device copies (through the plan's pinned slots, after whatever
  // still reads the old tables has drained)
  bool upload_filterbank(Filterbank& f)
  {
    f.layout = logic::filterbank_layout(tiles(), interior_lanes(), bins_per_lane(), f.bin0.size(), f.bin0.data(), f.nbins.data());
    const logic::FilterbankLayout& l = f.layout;
    if (!d_fb_pieces.reserve(l.pieces.size()) || !d_fb_tile0.reserve(l.tile_piece0.size()) || !d_fb_splits.reserve(l.splits.size()) ||
        !d_fb_weights.reserve(f.weights.size())) return false;
    std::vector<FD> tile_ordered(f.weights.size());          // the weights piece after piece (FilterbankPiece::woff)
    for (size_t i = 0; i < l.pieces.size(); ++i) std::copy_n(f.weights.data() + l.wsrc[i], l.pieces[i].nbins, tile_ordered.data() + l.pieces[i].woff);
    SDFT_TRY(hipStreamSynchronize(stream));
    if (!to_device(d_fb_pieces.p, l.pieces.data(), l.pieces.size() * sizeof(FilterbankPiece)) ||
        !to_device(d_fb_tile0.p, l.tile_piece0.data(), l.tile_piece0.size() * sizeof(unsigned)) ||
        !to_device(d_fb_splits.p, l.splits.data(), l.splits.size() * sizeof(FilterbankSplit)) ||
        !to_device(d_fb_weights.p, tile_ordered.data(), tile_ordered.size() * sizeof(FD))) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    f.interior = interior_lanes();
    return true;
  }
  // sdft_hip_set_filterbank: the arrays are host memory and are copied; a refused filterbank leaves the installed one as it is
  bool set_filterbank(size_t nbands, const size_t* band_bin0, const size_t* band_nbins, const FD* weights)
  {
    static const char* fn = "sdft_hip_set_filterbank";
    switch (logic::filterbank_check(nbins, nbands, band_bin0, band_nbins, weights != nullptr))
    {
      case logic::FB_OK: break;
      case logic::FB_NULL: set_error(fn, "band_bin0, band_nbins or weights is NULL but nbands is not 0"); return false;
      case logic::FB_EMPTY_BAND: set_error(fn, "a band has no bins (band_nbins[b] == 0)"); return false;
      case logic::FB_PAST_END: set_error(fn, "a band does not lie within the plan's bins (band_bin0[b] + band_nbins[b] > dftsize)"); return false;
      default: set_error(fn, "the filterbank is too large: 2^31 bands or 2^32 weights"); return false;
    }
    if (!bind()) return false;
    if (!pipe_join()) return false;
    Filterbank f;
    if (nbands)
    {
      f.bin0.assign(band_bin0, band_bin0 + nbands);
      f.nbins.assign(band_nbins, band_nbins + nbands);
      f.weights.assign(weights, weights + logic::filterbank_weights(nbands, band_nbins));
      if (!upload_filterbank(f)) { fbank.interior = -1; return false; }      // (the device tables are rebuilt from fbank by its next call)
    }
    else SDFT_TRY(hipStreamSynchronize(stream));
    fbank = std::move(f);
    return true;
  }
  size_t filterbank_bands() const { return fbank.bin0.size(); }

  // filterbank analysis (sdft_hip_sdft_filterbank_n): per band of the installed filterbank the sum of fl(weight * power) over the
  // band's bins, of the rows of the grid, dense [channels][rows][nbands] real numbers -- forward_filterbank_kernel, then
  // filterbank_rows_kernel for the bands a tile boundary cuts (forward_rows_stage: in as many launches as keep the workspace
  // within its bound)
  bool sdft_filterbank_n(size_t n, const TD* x, size_t every, size_t first, FD* out, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_filterbank_n";
    rows = 0;
    const size_t nbands = filterbank_bands();
    if (nbands == 0) { set_error(fn, "no filterbank is installed (sdft_hip_set_filterbank)"); return false; }
    if (!grid_args(fn, n, every, first, false, 0, 0, nullptr, false, out, "out", rows)) return false;
    last_filterbank_launches = 0;                            // (forward_rows_stage counts, over all host segments of the call)
    auto ready = [&] {                                       // (option "interior" changed the tiles)
      if (fbank.interior == interior_lanes() || upload_filterbank(fbank)) return true;
      fbank.interior = -1;
      return false;
    };
    return every_grid_call(n, x, every, first, out, rows, channels, nbands, ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
      const logic::FilterbankLayout& l = fbank.layout;
      const FilterbankArgs<FD> g{at, at_rows * nbands, nullptr, 0, 0, p.grid.every, p.grid.first, d_fb_pieces.p, d_fb_tile0.p,
                                 d_fb_weights.p, d_fb_splits.p, (unsigned)nbands, (unsigned)l.nslots, (unsigned)l.splits.size()};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::filterbank(g));
    });
  }

  // band-peak analysis (sdft_hip_sdft_band_peak_n): per band of the installed filterbank the largest fl(weight * power) over the
  // band's bins and the bin that attains it, of the rows of the grid, dense [channels][rows][nbands][2] real numbers --
  // forward_band_peak_kernel, then band_peak_rows_kernel for the bands a tile boundary cuts, in the filterbank call's launches by
  // rows with a pair per workspace slot (forward_rows_stage).  A unit row of every_grid_call is the 2 * nbands numbers of a row.
  bool sdft_band_peak_n(size_t n, const TD* x, size_t every, size_t first, FD* peaks, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_band_peak_n";
    rows = 0;
    const size_t nbands = filterbank_bands();
    if (nbands == 0) { set_error(fn, "no filterbank is installed (sdft_hip_set_filterbank)"); return false; }
    const char* const refused = logic::band_peak_bins_exact(nbins, sizeof(FD)) ? nullptr : "dftsize is beyond 2^24: a bin would not be an exact number of sdft_fd_t";
    if (!grid_args(fn, n, every, first, false, 0, 0, refused, false, peaks, "peaks", rows)) return false;
    last_band_peak_launches = 0;                             // (forward_rows_stage counts, over all host segments of the call)
    auto ready = [&] {                                       // (option "interior" changed the tiles: the pieces are cut again)
      if (fbank.interior == interior_lanes() || upload_filterbank(fbank)) return true;
      fbank.interior = -1;
      return false;
    };
    const size_t unit_row = logic::kBandPeakPair * nbands;
    return every_grid_call(n, x, every, first, peaks, rows, channels, unit_row, ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
      const logic::FilterbankLayout& l = fbank.layout;
      const FilterbankArgs<FD> g{at, at_rows * unit_row, nullptr, 0, 0, p.grid.every, p.grid.first, d_fb_pieces.p, d_fb_tile0.p,
                                 d_fb_weights.p, d_fb_splits.p, (unsigned)nbands, (unsigned)l.nslots, (unsigned)l.splits.size()};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::band_peak(g));
    });
  }

  // array-of-row-pointers variant (sdft.h:622-628).  Single-channel plans only: the reference's
  // table has one pointer per sample, a batched layout for it is not defined.
  bool single_channel(const char* fn)
  {
    if (channels == 1) return true;
    set_error(fn, "row-pointer variants take single-channel plans only (use sdft_sdft_n / sdft_isdft_n with a batched plan)");
    return false;
  }

  // pooled power analysis (sdft_hip_sdft_power_sum_n): the sums of sdft_power_n's every == 1 powers over the windows of the grid,
  // dense [channels][rows][nbins_out] real numbers -- forward_pooled_power_kernel, then pooled_power_rows_kernel for the windows
  // a chunk boundary cut; head rows in d_psum_head
  bool sdft_power_sum_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* sums, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_power_sum_n", n, every, first, true, bin0, nbins_out, nullptr, true, sums, "sums", rows)) return false;
    return pooled_grid_call(n, x, every, first, sums, rows, channels, nbins_out, d_psum_head, nullptr, kJoinAdd, grid_ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const PowerSumArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::power_sum(g));
    });
  }
  // peak-hold analysis (sdft_hip_sdft_power_peak_n): the largest (hold 0) or the smallest (hold 1) of those powers over the windows
  // of the grid; the pooled power call with forward_power_peak_kernel, peak_rows_kernel and peak_join_kernel in its kernels' places
  bool sdft_power_peak_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, int hold, FD* peaks, size_t& rows)
  {
    const char* const refused = logic::peak_hold_ok(hold) ? nullptr : "hold must be sdft_hip_hold_max (0) or sdft_hip_hold_min (1)";
    if (!grid_args("sdft_hip_sdft_power_peak_n", n, every, first, true, bin0, nbins_out, refused, true, peaks, "peaks", rows)) return false;
    return pooled_grid_call(n, x, every, first, peaks, rows, channels, nbins_out, d_psum_head, nullptr, hold, grid_ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const PowerSumArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::power_peak(g, hold));
    });
  }
  // smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n): the largest (hold 0) or the smallest (hold 1) over the windows of the
  // grid of sdft_power_smooth_n's sequence s, taken after every sample's step -- the peak-hold call's path (its head buffer, its
  // join of the segments' head rows) with forward_smooth_peak_kernel, and sdft_power_smooth_n's travel of s: from the caller's state
  // through the two halves of d_smooth_state, a forward call reading one and writing the other, the next segment of a call on host
  // memory going on from there, and back to the caller once the whole call has succeeded.  A call in several segments reports
  // their number as "last_segments".
  bool sdft_smooth_peak_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, double decay, int hold, FD* state,
                          FD* peaks, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_smooth_peak_n", n, every, first, true, bin0, nbins_out, logic::smooth_peak_refusal<FD>(hold, decay), true, peaks, "peaks", rows)) return false;
    if (n == 0 || nbins == 0) return true;
    const FD a = (FD)decay, b = (FD)1 - a;
    const size_t count = channels * nbins_out;
    bool state_device = false;
    int cur = 0;                                             // the half of d_smooth_state that holds s
    long pieces = 0;                                         // forward calls: more than one when host memory goes in segments
    auto ready = [&] {
      if (!d_smooth_state.reserve(2 * count)) return false;
      state_device = state && on_device(state);
      if (!state) SDFT_TRY(hipMemsetAsync(d_smooth_state.p, 0, count * sizeof(FD), stream));
      else if (state_device) SDFT_TRY(hipMemcpyAsync(d_smooth_state.p, state, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
      else if (!to_device(d_smooth_state.p, state, count * sizeof(FD))) return false;
      return true;
    };
    if (!pooled_grid_call(n, x, every, first, peaks, rows, channels, nbins_out, d_psum_head, nullptr, hold, ready,
                          [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
          const SmoothPeakArgs<FD> g{{row0, row0_stride, rest, rest_stride, nullptr, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out},
                                     d_smooth_state.p + cur * count, d_smooth_state.p + (cur ^ 1) * count, nullptr, a, b};
          if (!forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::smooth_peak(g, hold))) return false;
          cur ^= 1; ++pieces;
          return true;
        })) return false;
    if (pieces > 1) last_segments = pieces;                  // ("last_segments": the call went in that many time segments, each a call with its own carries)
    if (!state) return true;
    if (!state_device) return to_host(state, d_smooth_state.p + cur * count, count * sizeof(FD));
    SDFT_TRY(hipMemcpyAsync(state, d_smooth_state.p + cur * count, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
    return async || synchronize();
  }
  // ---- pooled cross-spectrum analysis ------------------------------------------------------------------------------------------
  // sdft_hip_set_pairs: the arrays are host memory and are copied; a refused list leaves the installed one as it is.  The work
  // items of the list (logic::cross_items) go to the device once, here.
  bool set_pairs(size_t npairs, const size_t* pair_a, const size_t* pair_b)
  {
    static const char* fn = "sdft_hip_set_pairs";
    switch (logic::cross_pairs_check(channels, npairs, pair_a, pair_b))
    {
      case logic::CX_OK: break;
      case logic::CX_NULL: set_error(fn, "pair_a or pair_b is NULL but npairs is not 0"); return false;
      case logic::CX_CHANNEL: set_error(fn, "a pair names a channel the plan does not have (index >= channels)"); return false;
      default: set_error(fn, "the list is too long: more than 2^31 pairs"); return false;
    }
    if (!bind()) return false;
    if (!pipe_join()) return false;
    Pairs f;
    if (npairs)
    {
      f.a.assign(pair_a, pair_a + npairs);
      f.b.assign(pair_b, pair_b + npairs);
      f.items = logic::cross_items(channels, npairs, pair_a, pair_b);
      // (a fresh table: whatever still reads the installed one has drained before it is replaced, and a failure leaves it alone)
      DevBuf<CrossItem> table;
      SDFT_TRY(hipStreamSynchronize(stream));
      if (!table.reserve(f.items.size())) return false;
      static_assert(sizeof(CrossItem) == sizeof(logic::CrossItem), "one table for the host and the kernel");
      if (!to_device(table.p, f.items.data(), f.items.size() * sizeof(CrossItem)) || hipStreamSynchronize(stream) != hipSuccess) { table.release(); return false; }
      d_cross_items.release();
      d_cross_items = table;
    }
    else SDFT_TRY(hipStreamSynchronize(stream));
    pairs = std::move(f);
    return true;
  }
  size_t pairs_count() const { return pairs.a.size(); }

  // pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n): per pair (a, b) of the installed list the sums of A conj(B) over the
  // windows of the grid, dense [npairs][rows][nbins_out] complex numbers -- forward_cross_sum_kernel, then pooled_power_rows_kernel
  // for the windows a chunk boundary cut.  The units are the pairs, not the channels: head rows in d_cross_head, the rows of a host
  // buffer through d_cross_stage.
  bool sdft_cross_sum_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* sums, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_cross_sum_n";
    rows = 0;
    const size_t npairs = pairs_count();
    if (npairs == 0) { set_error(fn, "no pairs are installed (sdft_hip_set_pairs)"); return false; }
    if (!grid_args(fn, n, every, first, true, bin0, nbins_out, nullptr, true, sums, "sums", rows)) return false;
    return pooled_grid_call(n, x, every, first, sums, rows, npairs, 2 * nbins_out, d_cross_head, &d_cross_stage, kJoinAdd, grid_ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const CrossSumArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, d_cross_items.p, (unsigned)pairs.items.size(), (unsigned)npairs,
                               p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::cross_sum(g));
    });
  }

  // smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n): per pair (a, b) of the installed list and per component of
  // A conj(B), s[t] = fl(fl(a * s[t - 1]) + fl(b * term[t])), advanced at every sample and kept on the grid, dense
  // [npairs][rows][nbins_out] complex numbers -- forward_cross_smooth_kernel, then, in a call of more than one chunk,
  // smooth_scan_kernel and smooth_fix_kernel over 2 * nbins_out real numbers per pair.  sdft_power_smooth_n's path with the pairs
  // for units: s travels through the two halves of d_cross_smooth_state, the rows of a host buffer through d_cross_smooth_stage
  // (the fix-up re-reads the rows it completes).
  bool sdft_cross_smooth_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, double decay, FD* state, FD* smooth,
                           size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_cross_smooth_n";
    rows = 0;
    const size_t npairs = pairs_count();
    if (npairs == 0) { set_error(fn, "no pairs are installed (sdft_hip_set_pairs)"); return false; }
    const char* const refused = logic::power_smooth_decay_ok<FD>(decay) ? nullptr : "decay must be at least 0 and less than 1 after rounding to sdft_fd_t";
    if (!grid_args(fn, n, every, first, true, bin0, nbins_out, refused, false, smooth, "smooth", rows)) return false;
    if (n == 0 || nbins == 0) return true;
    const FD a = (FD)decay, b = (FD)1 - a;
    const size_t unit_row = logic::cross_smooth_unit_row(nbins_out);
    const size_t count = npairs * unit_row;
    bool state_device = false;
    int cur = 0;                                             // the half of d_cross_smooth_state that holds s
    long pieces = 0;                                         // forward calls: more than one when host memory goes in segments
    auto ready = [&] {
      if (!d_cross_smooth_state.reserve(2 * count)) return false;
      state_device = state && on_device(state);
      if (!state) SDFT_TRY(hipMemsetAsync(d_cross_smooth_state.p, 0, count * sizeof(FD), stream));
      else if (state_device) SDFT_TRY(hipMemcpyAsync(d_cross_smooth_state.p, state, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
      else if (!to_device(d_cross_smooth_state.p, state, count * sizeof(FD))) return false;
      return true;
    };
    if (!every_grid_call(n, x, every, first, smooth, rows, npairs, unit_row, ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
          const CrossSmoothArgs<FD> g{at, logic::power_channel_stride(at_rows, unit_row), d_cross_smooth_state.p + cur * count,
                                      d_cross_smooth_state.p + (cur ^ 1) * count, nullptr, d_cross_items.p, (unsigned)pairs.items.size(), (unsigned)npairs,
                                      a, b, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
          if (!forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::cross_smooth(g))) return false;
          cur ^= 1; ++pieces;
          return true;
        }, &d_cross_smooth_stage)) return false;
    if (pieces > 1) last_segments = pieces;                  // (as sdft_power_smooth_n reports them)
    if (!state) return true;
    if (!state_device) return to_host(state, d_cross_smooth_state.p + cur * count, count * sizeof(FD));
    SDFT_TRY(hipMemcpyAsync(state, d_cross_smooth_state.p + cur * count, count * sizeof(FD), hipMemcpyDeviceToDevice, stream));
    return async || synchronize();
  }

  // lag-product analysis (sdft_hip_sdft_lag_sum_n): per channel the sums of X[t] conj(X[t - 1]) over the windows of the grid, dense
  // [channels][rows][nbins_out] complex numbers.  The cross-spectrum call above with the plan's channels in the pairs' place -- its
  // arguments (no items), workspace, head and stage buffers -- and forward_lag_sum_kernel, which steps one recurrence per wave on the
  // pooled power call's route.  The row before a call's (and so a segment's) first sample is the row of the state the call starts
  // from, which the kernel demodulates itself: a later segment's first term needs nothing from this side.
  bool sdft_lag_sum_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* sums, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_lag_sum_n", n, every, first, true, bin0, nbins_out, nullptr, true, sums, "sums", rows)) return false;
    return pooled_grid_call(n, x, every, first, sums, rows, channels, 2 * nbins_out, d_cross_head, &d_cross_stage, kJoinAdd, grid_ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const CrossSumArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, nullptr, (unsigned)channels, (unsigned)channels,
                               p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::lag_sum(g));
    });
  }

  // power-moments analysis (sdft_hip_sdft_power_moments_n): per channel the pairs (sum of the power, sum of its square) over the
  // windows of the grid, dense [channels][rows][nbins_out][2] real numbers.  The lag-product call's host side -- the cross-spectrum
  // call's arguments with the plan's channels in the pairs' place, its workspace, head and stage buffers, the pooled adders over
  // 2 * nbins_out numbers -- and forward_power_moments_kernel on the pooled power call's route and chunk choice.
  bool sdft_power_moments_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* moments, size_t& rows)
  {
    if (!grid_args("sdft_hip_sdft_power_moments_n", n, every, first, true, bin0, nbins_out, nullptr, true, moments, "moments", rows)) return false;
    return pooled_grid_call(n, x, every, first, moments, rows, channels, 2 * nbins_out, d_cross_head, &d_cross_stage, kJoinAdd, grid_ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const CrossSumArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, nullptr, (unsigned)channels, (unsigned)channels,
                               p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::power_moments(g));
    });
  }

  // ---- array covariance analysis ------------------------------------------------------------------------------------------------
  // sdft_hip_set_array: the list is host memory and is copied (nullptr: the channels 0 ... nch - 1); a refused list leaves the
  // installed one as it is.  The work items (logic::covariance_items) and the list go to the device here, and again when a test
  // hook changes the group size (upload_array).
  bool upload_array(Array& f)
  {
    f.group = array_group();
    f.items = logic::covariance_items(channels, f.chan.size(), f.chan.data(), f.group);
    std::vector<unsigned> chan32(f.chan.begin(), f.chan.end());
    // (fresh tables: whatever still reads the installed ones has drained before they are replaced, and a failure leaves them alone)
    DevBuf<CovItem> table;
    DevBuf<unsigned> list;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (!table.reserve(f.items.size()) || !list.reserve(chan32.size())) { table.release(); list.release(); return false; }
    if (!to_device(table.p, f.items.data(), f.items.size() * sizeof(CovItem)) || !to_device(list.p, chan32.data(), chan32.size() * sizeof(unsigned)) ||
        hipStreamSynchronize(stream) != hipSuccess) { table.release(); list.release(); return false; }
    d_cov_items.release(); d_cov_chan.release();
    d_cov_items = table; d_cov_chan = list;
    return true;
  }
  bool set_array(size_t nch, const size_t* chan)
  {
    static const char* fn = "sdft_hip_set_array";
    switch (logic::array_check(channels, nch, chan))
    {
      case logic::AR_OK: break;
      case logic::AR_CHANNEL: set_error(fn, "the list names a channel the plan does not have (index >= channels)"); return false;
      case logic::AR_REPEAT: set_error(fn, "the list names a channel twice"); return false;
      default: set_error(fn, "the list is too long: more channels than the plan has (or than 65535)"); return false;
    }
    if (!bind()) return false;
    if (!pipe_join()) return false;
    Array f;
    if (nch)
    {
      f.chan.resize(nch);
      for (size_t i = 0; i < nch; ++i) f.chan[i] = chan ? chan[i] : i;
      if (!upload_array(f)) return false;
    }
    else SDFT_TRY(hipStreamSynchronize(stream));
    array = std::move(f);
    return true;
  }
  size_t array_channels() const { return array.chan.size(); }

  // array covariance analysis (sdft_hip_sdft_covariance_n): sdft_cross_sum_n for all pairs (i <= j) of the installed array, dense
  // [nch (nch + 1) / 2][rows][nbins_out] complex numbers in the order of logic::covariance_pair_index (head rows in d_cov_head, the
  // rows of a host buffer through d_cov_stage); forward_covariance_kernel forms the sums by blocks of groups of channels
  bool sdft_covariance_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* sums, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_covariance_n";
    rows = 0;
    const size_t nch = array_channels(), npairs = logic::covariance_pairs(nch);
    if (nch == 0) { set_error(fn, "no array is installed (sdft_hip_set_array)"); return false; }
    if (!grid_args(fn, n, every, first, true, bin0, nbins_out, nullptr, true, sums, "cov", rows)) return false;
    auto ready = [&] { return array.group == array_group() || upload_array(array); };      // (a test hook changed the group size)
    return pooled_grid_call(n, x, every, first, sums, rows, npairs, 2 * nbins_out, d_cov_head, &d_cov_stage, kJoinAdd, ready,
                            [&](const GridPiece& p, FD* row0, size_t row0_stride, FD* rest, size_t rest_stride) {
      const CovarianceArgs<FD> g{row0, row0_stride, rest, rest_stride, nullptr, d_cov_items.p, d_cov_chan.p, (unsigned)array.items.size(), (unsigned)nch,
                                 (unsigned)npairs, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::covariance(g));
    });
  }

  // ---- channel-mix analysis ---------------------------------------------------------------------------------------------------------
  // sdft_hip_set_mix: list and weights are host memory and are copied (chan == nullptr: the channels 0 ... nch - 1); a refused mix
  // leaves the installed one as it is.  The work items (logic::mix_items) go to the device here, and again when a test hook changes
  // the block size (upload_mix_items); the weight table [nout][nch][N] does not depend on it.
  bool upload_mix_items(Mix& f, DevBuf<MixItem>& into)
  {
    f.block = mix_block_size();
    f.items = logic::mix_items(channels, f.chan.size(), f.chan.data(), f.nout, f.block);
    DevBuf<MixItem> table;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (!table.reserve(f.items.size())) return false;
    if (!to_device(table.p, f.items.data(), f.items.size() * sizeof(MixItem)) || hipStreamSynchronize(stream) != hipSuccess) { table.release(); return false; }
    into.release();
    into = table;
    return true;
  }
  bool set_mix(size_t nout, size_t nch, const size_t* chan, const fdx* weights)
  {
    static const char* fn = "sdft_hip_set_mix";
    switch (logic::mix_check(channels, nout, nch, chan, weights != nullptr))
    {
      case logic::MX_OK: break;
      case logic::MX_NO_WEIGHTS: set_error(fn, "weights is NULL"); return false;
      case logic::MX_NO_CHANNELS: set_error(fn, "a mix needs at least one channel (nch == 0)"); return false;
      case logic::MX_CHANNEL: set_error(fn, "the list names a channel the plan does not have (index >= channels)"); return false;
      case logic::MX_REPEAT: set_error(fn, "the list names a channel twice"); return false;
      case logic::MX_TOO_MANY_OUTPUTS: set_error(fn, "too many outputs (more than 65535)"); return false;
      default: set_error(fn, "the list is too long: more channels than the plan has (or than 65535)"); return false;
    }
    if (!bind()) return false;
    if (!pipe_join()) return false;
    Mix f;
    if (nout)
    {
      f.nout = nout;
      f.chan.resize(nch);
      for (size_t i = 0; i < nch; ++i) f.chan[i] = chan ? chan[i] : i;
      std::vector<unsigned> chan32(f.chan.begin(), f.chan.end());
      // (fresh tables: whatever still reads the installed ones has drained before they are replaced, and a failure leaves them alone)
      const size_t count = nout * nch * nbins;
      if (nbins && count / nbins / nch != nout) { set_error(fn, "the weight table cannot be reserved"); return false; }
      DevBuf<MixItem> table;
      DevBuf<unsigned> list;
      DevBuf<fdx> wtable;
      auto drop = [&] { table.release(); list.release(); wtable.release(); return false; };
      if (!list.reserve(chan32.size()) || !wtable.reserve(std::max<size_t>(count, 1))) return drop();
      if (!upload_mix_items(f, table)) return drop();
      if (!to_device(list.p, chan32.data(), chan32.size() * sizeof(unsigned)) || !to_device(wtable.p, weights, count * sizeof(fdx)) ||
          hipStreamSynchronize(stream) != hipSuccess) return drop();
      d_mix_items.release(); d_mix_chan.release(); d_mix_weights.release();
      d_mix_items = table; d_mix_chan = list; d_mix_weights = wtable;
    }
    else
    {
      SDFT_TRY(hipStreamSynchronize(stream));
      d_mix_items.release(); d_mix_chan.release(); d_mix_weights.release();
    }
    mix = std::move(f);
    return true;
  }
  size_t mix_outputs() const { return mix.nout; }

  // channel-mix analysis (sdft_hip_sdft_mix_n): the weighted sums of the installed mix at the rows of the grid, for the bins of
  // sdft_power_n's band, dense [nout][rows][nbins_out] complex numbers -- forward_mix_kernel.  Rows on their way to a host buffer
  // are formed in d_mix_stage, so that the kernel never re-reads a running sum from host memory, and copied out output by output.
  bool sdft_mix_n(size_t n, const TD* x, size_t every, size_t first, size_t bin0, size_t nbins_out, FD* out, size_t& rows)
  {
    static const char* fn = "sdft_hip_sdft_mix_n";
    rows = 0;
    const size_t nout = mix.nout, nch = mix.chan.size();
    if (nout == 0) { set_error(fn, "no mix is installed (sdft_hip_set_mix)"); return false; }
    if (!grid_args(fn, n, every, first, true, bin0, nbins_out, nullptr, false, out, "out", rows)) return false;
    auto ready = [&] { return mix.block == mix_block_size() || upload_mix_items(mix, d_mix_items); };      // (a test hook changed the block size)
    return every_grid_call(n, x, every, first, out, rows, nout, 2 * nbins_out, ready, [&](const GridPiece& p, FD* at, size_t at_rows) {
      const MixArgs<FD> g{at, logic::mix_output_stride(at_rows, nbins_out), d_mix_weights.p, d_mix_items.p, d_mix_chan.p, (unsigned)mix.items.size(), (unsigned)nch,
                          (unsigned)nout, p.grid.every, p.grid.first, (unsigned)bin0, (unsigned)nbins_out};
      return forward_device(p.m, p.td, p.td_stride, nullptr, 0, nullptr, ForwardCall::channel_mix(g));
    }, &d_mix_stage);
  }

  // a host table of device rows goes to the device; nullptr: failed
  fdx* const* device_table(fdx* const* dfts, size_t n, bool table_on_device)
  {
    if (table_on_device) return dfts;
    if (!d_rowptr.reserve(n) || !to_device(d_rowptr.p, dfts, n * sizeof(fdx*))) return nullptr;
    return d_rowptr.p;
  }
  bool sdft_nd(size_t n, const TD* x, fdx** dfts)
  {
    if (n == 0 || nbins == 0) return true;
    if (!single_channel("sdft_sdft_nd")) return false;
    if (!bind()) return false;
    const bool table_on_device = is_device_pointer(dfts);
    if (table_on_device || is_device_pointer(dfts[0]))
    {
      // rows live on the device: hand the pointer table to the kernel
      fdx* const* table = device_table(dfts, n, table_on_device);
      if (!table) return false;
      const TD* xs = is_device_pointer(x) ? x : staged_samples(x, n);
      return xs && forward_device(n, xs, n, nullptr, 0, table) && synchronize();
    }
    // host rows: compute dense segments, scatter row by row
    const size_t seg = logic::stage_rows(n, nbins * sizeof(fdx), stage_bytes);
    std::vector<fdx> host(seg * nbins);
    Scoped<bool> sync(async, false);
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      if (!sdft_n(m, x + t, host.data())) return false;
      for (size_t r = 0; r < m; ++r) memcpy(dfts[t + r], host.data() + r * nbins, nbins * sizeof(fdx));
    }
    return true;
  }

  // empty spectrum: the reference returns (td)(0 * 2)
  bool zero_samples(size_t n, TD* y, bool yd)
  {
    if (yd) SDFT_TRY(hipMemsetAsync(y, 0, channels * n * sizeof(TD), stream)); else memset(y, 0, channels * n * sizeof(TD));
    return finish();
  }
  // y_class: -1 = classify y, 0 = y is host memory whatever option "pointers" says (the by-value result of sdft_isdft)
  bool isdft_n(size_t n, const fdx* dfts, TD* y, int y_class = -1)
  {
    if (n == 0) return true;
    if (opt_resident && y_class < 0 && resident_synthesis(n, dfts, y)) return true;
    if (!bind()) return false;
    const bool id = on_device(dfts);
    const bool yd = y_class < 0 ? on_device(y) : y_class != 0;
    if (nbins == 0) return zero_samples(n, y, yd);
    TD* y_map = nullptr; fdx* i_map = nullptr;
    const logic::HostRoute r = host_route(false, n, y, yd, y_class == 0, dfts, id, y_map, i_map);
    if (r.refused) return copy_failed();
    if (r.route == logic::HR_STAGED)
      return staged_segments(n, r.seg, StagedCall{false, y, !yd, const_cast<fdx*>(dfts), !id, n, r.seg, bins_row_bytes()},
                             [&](Segment& s) { return inverse_device(s.m, s.bins(), s.mat_rows * nbins, nullptr, s.td, s.td_stride); });
    const size_t ibytes = matrix_bytes(n), ybytes = channels * n * sizeof(TD);
    const bool direct = r.route == logic::HR_DIRECT;
    double t1 = 0.0;
    if (direct)
    {
      // the host copies the matrix into the plan's pinned pieces, which the kernel reads over PCIe
      const double t0 = HostIo::now_us();
      io.copy_bytes(io.h_pin, dfts, ibytes);
      t1 = HostIo::now_us();
      io.pin_us_memcpy += t1 - t0;
      ++io.pin_copies;
    }
    // (the route has asked ensure_io already, before the copy above: it allocates on a plan's first such call only)
    TD* ys = r.samples == logic::HS_MAPPED ? y_map : r.samples == logic::HS_IO ? d_io : y;
    if (r.samples == logic::HS_STAGE_TD) { if (!d_stage_td.reserve(channels * n)) return false; ys = d_stage_td.p; }
    const fdx* in = direct ? reinterpret_cast<const fdx*>(io.d_pin) : (id ? dfts : i_map);
    Scoped<bool> sync(async, async && !r.synchronous), flag(flag_wanted, r.flag_wanted), pipe(pipe_allowed, r.pipe_allowed);   // (as in sdft_n)
    if (!inverse_device(n, in, n * nbins, nullptr, ys, n)) return false;
    if (r.samples == logic::HS_STAGE_TD && !to_host(y, ys, ybytes)) return false;
    if (!(r.end == logic::HE_FINISH ? finish(ibytes) : finish_mapped(ibytes))) return false;
    if (direct) io.pin_us_device += HostIo::now_us() - t1;
    if (r.samples == logic::HS_IO) memcpy(y, h_io, ybytes);   // the kernel wrote the samples into the pinned scratch
    return true;
  }

  bool isdft_nd(size_t n, const fdx** dfts, TD* y)
  {
    if (n == 0) return true;
    if (!single_channel("sdft_isdft_nd")) return false;
    if (!bind()) return false;
    if (nbins == 0) return isdft_n(n, nullptr, y);
    const bool table_on_device = is_device_pointer(dfts);
    if (table_on_device || is_device_pointer(dfts[0]))
    {
      const fdx* const* table = device_table(const_cast<fdx* const*>(dfts), n, table_on_device);
      if (!table) return false;
      TD* yy = y;
      const bool yd = is_device_pointer(y);
      if (!yd) { if (!d_stage_td.reserve(n)) return false; yy = d_stage_td.p; }
      if (!inverse_device(n, nullptr, 0, table, yy, n)) return false;
      if (!yd && !to_host(y, yy, n * sizeof(TD))) return false;
      return synchronize();
    }
    const size_t seg = logic::stage_rows(n, nbins * sizeof(fdx), stage_bytes);
    std::vector<fdx> host(seg * nbins);
    Scoped<bool> sync(async, false);
    for (size_t t = 0; t < n; t += seg)
    {
      const size_t m = std::min(seg, n - t);
      for (size_t r = 0; r < m; ++r) memcpy(host.data() + r * nbins, dfts[t + r], nbins * sizeof(fdx));
      if (!isdft_n(m, host.data(), y + t)) return false;
    }
    return true;
  }

  // single-sample synthesis (sdft.h:635): the result comes back by value, so a device-resident
  // row needs a one-element device buffer (owned by the plan, allocated on the plan's device)
  bool isdft_one(const fdx* dft, TD* y)
  {
    if (nbins == 0) { *y = (TD)0; return true; }           // the reference returns (td)(0 * 2)
    if (opt_resident && resident_synthesis_sample(dft, y)) return true;
    if (!bind()) return false;
    Scoped<bool> sync(async, false);
    return isdft_n(1, dft, y, 0);                            // (a device row: through the pinned scratch, see isdft_n; y lives on the host stack)
  }

  // ---- fused analysis -> spectral operation -> synthesis (SURVEY.md 8 f2) ------------------------
  // y[t] = sdft_isdft( op( sdft_sdft(x[t]) ) ) with the reference's arithmetic, without the (n, N)
  // matrix ever reaching HBM unless the caller asks for a copy of the processed spectrum in `dfts`.
  // params: OP_GAIN -> FD gains[N], OP_CGAIN -> cx<FD> gains[N] (host or device memory), OP_SHIFT -> const long* (host).
  DevBuf<FD> d_gain;
  DevBuf<TD> d_stage_y;
  bool wants_reference_order() const { return logic::reference_order(opt_fused_exact, carry_mode == CARRY_EXACT, sizeof(FD)); }

  // the call's operation: public operation numbers (enum sdft_hip_op: 0 identity, 1 gain, 2 shift, 3 cgain, 4 gain_rows, 5 cgain_rows,
  // 6 gate, 7 power, 8 expression) to the kernels' SpectralOp, parameters checked, gains on the device.  build == false (an
  // empty spectrum has no operation): only the checks that do not depend on the spectrum.
  bool process_op(int op_public, const void* params, const fdx* dfts, bool build, SpectralOp<FD>& op)
  {
    static const char* fn = "sdft_hip_process_n";
    if (op_public < 0 || op_public > 8) { set_error(fn, "unknown operation"); return false; }
    if ((op_public != 0) && !params) { set_error(fn, "the operation needs parameters"); return false; }
    const int op_kind = op_public == 4 ? OP_GAIN : op_public == 5 ? OP_CGAIN : op_public == 6 ? OP_GATE : op_public == 7 ? OP_POWER : op_public == 8 ? OP_USER : op_public;
    if (op_kind == OP_SHIFT && dfts) { set_error(fn, "a copy of the spectrum is not available with the shift operation"); return false; }
    if (!build) return true;
    if (dfts && !on_device(dfts)) { set_error(fn, "dfts must be device memory (or NULL)"); return false; }
    op.kind = op_kind; op.gain = nullptr; op.shift = 0; op.rows = 1; op.hop = 0; op.t0 = 0;
    if (op_kind == OP_GAIN || op_kind == OP_CGAIN)
    {
      const FD* g = static_cast<const FD*>(params);
      size_t rows = 1;
      if (op_public >= 4)
      {
        // time-varying gains: { gains, rows, hop } (sdft_hip_gain_rows_t)
        struct table_t { const void* gains; size_t rows, hop; };
        const table_t* tb = static_cast<const table_t*>(params);
        if (!tb->gains || tb->rows == 0 || (tb->rows > 1 && tb->hop == 0)) { set_error(fn, "gain table: gains, rows >= 1 and hop >= 1 are required"); return false; }
        if (tb->rows > 0xffffffffull) { set_error(fn, "gain table: too many rows"); return false; }
        g = static_cast<const FD*>(tb->gains); rows = tb->rows; op.rows = (unsigned)rows; op.hop = tb->hop;
      }
      const size_t per_bin = op_kind == OP_CGAIN ? 2 : 1;          // real factors, or (re, im) pairs
      if (!on_device(g))
      {
        if (!d_gain.reserve(rows * nbins * 2)) return false;
        if (!to_device(d_gain.p, g, rows * nbins * per_bin * sizeof(FD))) return false;
        g = d_gain.p;
      }
      op.gain = g;
    }
    else if (op_kind == OP_SHIFT) op.shift = *static_cast<const long*>(params);
    else if (op_kind == OP_GATE || op_kind == OP_POWER) { const FD* q = static_cast<const FD*>(params); op.p0 = q[0]; op.p1 = q[1]; }   // host memory
    else if (op_kind == OP_USER)
    {
      // { expr, p, np }: the parameters travel to the device with the call (host memory; np may be 0)
      struct expr_t { const char* expr; const void* p; size_t np; };
      const expr_t* ex = static_cast<const expr_t*>(params);
      if (!ex->expr || !*ex->expr) { set_error(fn, "expression: no statements"); return false; }
      user_expr = ex->expr;
      if (ex->np <= 8)
      {
        // up to eight parameters ride in the kernel arguments (SpectralOp::pv)
        for (size_t i = 0; i < ex->np; ++i) op.pv[i] = static_cast<const FD*>(ex->p)[i];
      }
      else
      {
        if (!d_gain.reserve(ex->np)) return false;
        if (!to_device(d_gain.p, ex->p, ex->np * sizeof(FD))) return false;
        op.gain = d_gain.p;
      }
    }
    return true;
  }

  bool process_n(size_t n, const TD* x, TD* y, int op_kind, const void* params, fdx* dfts)
  {
    if (n == 0) return true;
    if (!bind()) return false;
    SpectralOp<FD> op{};
    if (nbins == 0) return process_op(op_kind, params, dfts, false, op) && zero_samples(n, y, on_device(y));
    if (!process_op(op_kind, params, dfts, true, op)) return false;
    const bool yd = on_device(y);
    // the samples: device pointers as they are, host pointers staged (4 bytes per sample each way)
    const bool xd = on_device(x);
    const TD* xs = x;
    if (!xd && !(xs = staged_samples(x, channels * n))) return false;
    TD* ys = y;
    if (!yd) { if (!d_stage_y.reserve(channels * n)) return false; ys = d_stage_y.p; }
    // In place (out == samples) or overlapping device buffers: the two reference calls read every sample before the first
    // output sample is written, the one-launch forms do not (workgroups read the samples of earlier chunks -- fold, delay
    // line, differences -- while others write their outputs).  The samples are copied aside first: 4-8 bytes per sample.
    if (xs == x && yd)
    {
      const uintptr_t xa = reinterpret_cast<uintptr_t>(xs), ya = reinterpret_cast<uintptr_t>(ys), bytes = channels * n * sizeof(TD);
      if (xa < ya + bytes && ya < xa + bytes)
      {
        if (!d_stage_td.reserve(channels * n)) return false;
        SDFT_TRY(hipMemcpyAsync(d_stage_td.p, xs, bytes, hipMemcpyDeviceToDevice, stream));
        xs = d_stage_td.p;
      }
    }
    // the route: every input is a quantity of the plan or an option, but for the device's free memory
    logic::ProcessQuery q;
    q.chunk = chunk_query(n, rows_kernel_ok(false)); q.fd_bytes = sizeof(FD); q.fdx_bytes = sizeof(fdx);
    q.linear = op_is_linear<FD>(op.kind); q.user = op.kind == OP_USER; q.gain_rows = op.rows;
    q.spectrum = dfts != nullptr; q.x_device = xd; q.y_device = yd;
    q.fused_exact = opt_fused_exact; q.fold = opt_fold; q.hop_kernel = opt_hop_kernel;
    q.exact_inverse = opt_exact_inverse; q.inverse_rows = opt_inverse_rows;
    q.stage_bytes = stage_bytes; q.workspace = d_stage_fdx.cap;
    const logic::ProcessRoute r = logic::process_route(q, [] {
      size_t free_b = 0, total_b = 0;
      const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
      (void)hipGetLastError();
      return known ? free_b : (size_t)0;
    });
    {
      Scoped<bool> flag(flag_wanted, r.flag_wanted);         // (read by the launches only: arm_flag, hop_parts -- not by fold_coefficients)
      if (r.path == logic::PP_HOP_FOLDED)
      {
        if (!fold_coefficients(op)) return false;
        last_process_path = 1;
        if (!coeff_ready || !process_hop(n, xs, n, ys, n)) return false;
      }
      else if (r.path == logic::PP_FUSED_ROWS)
      {
        FuseArgs<TD, FD> fz{};
        fz.y = ys; fz.y_stride = n; fz.syn = d_syn.p; fz.sweight = tab.sweight; fz.op = op; fz.store = dfts ? 1 : 0;
        fz.walked = walked_counter();
        if (r.fold) { if (!fold_coefficients(op)) return false; } else coeff_ready = false;
        last_process_path = 1;
        if (!forward_device(n, xs, n, dfts, n * nbins, nullptr, ForwardCall::fused(fz))) return false;
      }
      else
      {
        // two passes in segments of r.seg rows: analysis, then synthesis with the operation applied on the way in
        // (batched plans take segments too: the workspace's channel stride is the segment, mstride below)
        if (!dfts && !d_stage_fdx.reserve(channels * nbins * r.seg)) return false;
        last_process_path = r.path;                            // PP_HOP_PAIR = 2, PP_SEGMENTS = 3
        last_fused_exact = 0; last_fused_fold = 0;
        // every run-time-compiled kernel the segments below will ask for is resolved BEFORE the first launch: statements
        // that do not compile must not leave the stream advanced by an analysis whose synthesis then fails
        if (r.rtc_hop || r.rtc_rows)
        {
          hipFunction_t fn = nullptr;
          char hop_name[160], rows_name[96];
          snprintf(hop_name, sizeof(hop_name), "sdfthip::inverse_row_kernel<%s, %s, %s, true>", type_name<TD>(), type_name<FD>(), latency == 1 ? "true" : "false");
          snprintf(rows_name, sizeof(rows_name), "sdfthip::user_rows_kernel<%s>", type_name<FD>());
          if (r.rtc_hop && !rtc_kernel(user_expr.c_str(), hop_name, device, &fn)) return false;
          if (r.rtc_rows && !rtc_kernel(user_expr.c_str(), rows_name, device, &fn)) return false;
        }
        const bool user = op.kind == OP_USER, user_hop_form = user && opt_exact_inverse && opt_inverse_rows <= 0;
        for (size_t t = 0; t < n; t += r.seg)
        {
          const size_t m = std::min(r.seg, n - t);
          fdx* mat = dfts ? dfts + t * nbins : d_stage_fdx.p;
          const size_t mstride = dfts ? n * nbins : m * nbins;
          SpectralOp<FD> ops = op; ops.t0 = t;                  // gain vectors count from the start of the call
          // the operation runs inside the synthesis -- the host's own statements only on a hop (row synthesis, two launches):
          // on longer segments they rewrite the stored rows in place first, then plain synthesis
          const bool in_synthesis = !user || (user_hop_form && channels * m <= 1024);
          if (!forward_device(m, xs + t, n, mat, mstride, nullptr)) return false;
          if (!in_synthesis && !user_rows(mat, mstride, m, ops)) return false;
          if (!inverse_device(m, mat, mstride, nullptr, ys + t, n, in_synthesis ? &ops : nullptr)) return false;
          // a copy of the spectrum is processed afterwards
          if (in_synthesis && dfts && user && !user_rows(mat, mstride, m, ops)) return false;
          if (in_synthesis && dfts && (op.kind == OP_GAIN || op.kind == OP_CGAIN || (op.kind >= OP_GATE && !user)) && !scale_rows(mat, mstride, m, ops)) return false;
        }
      }
    }
    if (!yd)
    {
      if (!to_host(y, ys, channels * n * sizeof(TD))) return false;
      return synchronize();
    }
    // (the fused call moves the samples only -- unless the host asked for a copy of the spectrum or the shape took the two passes)
    return finish((dfts || last_process_path != 1) ? matrix_bytes(n) : std::max<size_t>(1, channels * n * 2 * sizeof(TD)));
  }

  // the host's own operation on stored rows (two-pass route): user_rows_kernel compiled at run time with its statements
  bool user_rows(fdx* mat, size_t stride, size_t rows, const SpectralOp<FD>& op)
  {
    char name[96];
    snprintf(name, sizeof(name), "sdfthip::user_rows_kernel<%s>", type_name<FD>());
    hipFunction_t fn = nullptr;
    if (!rtc_kernel(user_expr.c_str(), name, device, &fn)) return false;
    if (!pipe_join()) return false;
    const size_t total = channels * rows * nbins;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    fdx* a0 = mat; size_t a1 = stride, a2 = rows; unsigned a3 = (unsigned)nbins, a4 = (unsigned)channels; SpectralOp<FD> a5 = op;
    void* args[] = {&a0, &a1, &a2, &a3, &a4, &a5};
    SDFT_TRY(hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
    return true;
  }

  // processed copy of the spectrum on the two-pass path: rows *= gain (the fused kernel stores them scaled)
  bool scale_rows(fdx* mat, size_t stride, size_t rows, const SpectralOp<FD>& op)
  {
    if (!pipe_join()) return false;
    const size_t total = channels * rows * nbins;
    const unsigned blocks = (unsigned)std::min<size_t>((total + kBlock - 1) / kBlock, 65536);
    hipLaunchKernelGGL((scale_rows_kernel<FD>), dim3(blocks), dim3(kBlock), 0, stream, mat, stride, rows, (unsigned)nbins, (unsigned)channels, op);
    SDFT_TRY(hipGetLastError());
    return true;
  }

  // checkpoint / resume: install a state previously read with get_state (any plan of the same
  // dftsize, window, latency, types and channel count -- also on another GPU)
  bool set_state(const fdx* acc, const fdx* fid, const TD* hist, size_t cur)
  {
    if (!bind()) return false;
    if (!pipe_join()) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (nbins)
    {
      if (cur >= 2 * nbins) { set_error("sdft_hip_set_state", "cursor out of range"); return false; }
      if (acc && !to_device(acc_p(), acc, channels * nbins * sizeof(fdx))) return false;
      if (fid) { if (!to_device(fid_p(), fid, channels * nbins * sizeof(fdx))) return false; fid_canonical = false; }
      if (hist && !to_device(d_hist[hist_cur].p, hist, channels * 2 * nbins * sizeof(TD))) return false;
      SDFT_TRY(hipStreamSynchronize(stream));
    }
    cursor = cur;
    return true;
  }

  // state read-back for tests: acc, fid [channels][N]; hist [channels][2N] in time order
  bool get_state(fdx* acc, fdx* fid, TD* hist, size_t* cur)
  {
    if (!bind()) return false;
    if (!pipe_join()) return false;
    SDFT_TRY(hipStreamSynchronize(stream));
    if (nbins)
    {
      if (acc && !to_host(acc, acc_p(), channels * nbins * sizeof(fdx))) return false;
      if (fid && !to_host(fid, fid_p(), channels * nbins * sizeof(fdx))) return false;
      if (hist && !to_host(hist, d_hist[hist_cur].p, channels * 2 * nbins * sizeof(TD))) return false;
      SDFT_TRY(hipStreamSynchronize(stream));
    }
    if (cur) *cur = cursor;
    return true;
  }
