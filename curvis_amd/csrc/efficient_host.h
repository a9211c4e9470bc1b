/* efficient_host.h -- host side of render_image_efficient (E1-E4): batched escape-angle evaluation, the adaptive sampler
 * driver with speculation, the device sampler's slots and prefetch, per-pixel launch; direct mode; trajectories.
 * Part of the ONE translation unit curvis_hip.hip (included there, nowhere else). */
#pragma once

namespace {

/* ---- efficient mode ------------------------------------------------------------------------- */

/* what the three entry points of the efficient renderer are given (render, render batch, prefetch) */
struct EfficientCall {
  const curvis_metric *metric;
  const curvis_camera *cams;
  uint32_t n_frames, max_iter;
  double max_radius, delta;
  uint32_t alpha_nums, max_iterations_sampling;
  double thr1, thr2;
  uint32_t filter = 0; /* option "sky_filter" for this call */
  uint32_t projection = 0; /* option "projection" for this call (CallShape: with PROJ_BOOSTED while a frame moves) */
  const cvk::CameraBoost *boost = nullptr; /* ... and then the frames' boosts, n_frames of them */
  uint32_t ss = 1; /* supersampling factor: with ss > 1 `cams` are those of the ss times finer pixel grid (render_efficient_impl) */
  double kappa = 0.0; /* option "step_scale" for this call: RN(delta / L0) ... */
  int adapt = 0; /* ... and the kernels' ADAPT (CallShape): 1 the samplers integrate with step_delta, 2 option "integrator" = 1, with Heun steps */
};

/* evaluate compute_escape_angle for a batch on the GPU */
int eval_escape_batch(curvis_ctx *ctx, const curvis_metric *metric, const cvk::MetricParams &MP,
                      const std::vector<double> &alpha, const std::vector<double> &lcam, uint32_t max_iter,
                      double max_radius, double delta, std::vector<double> &angle, std::vector<double> &space,
                      std::vector<uint32_t> &steps, std::vector<int> &status, double *ms_acc, int adapt = 0, double kappa = 0.0) {
  const size_t n = alpha.size();
  angle.resize(n);
  space.resize(n);
  steps.resize(n);
  status.resize(n);
  if (n == 0) return CURVIS_OK;
  /* layout: alpha | l | angle | space (f64) | steps (u32) | status (i32) */
  const size_t bytes = n * (4 * sizeof(double) + sizeof(unsigned) + sizeof(int));
  int rc = ctx->d_eff.reserve(ctx, bytes);
  if (rc) return rc;
  double *d_alpha = (double *)ctx->d_eff.p, *d_l = d_alpha + n, *d_angle = d_l + n, *d_space = d_angle + n;
  unsigned *d_steps = (unsigned *)(d_space + n);
  int *d_status = (int *)(d_steps + n);
  /* one pinned staging buffer, one copy in and one copy out per launch: pageable hipMemcpyAsync of more than
   * 1 MiB takes a path that costs ~10 ms per array on this stack (a 262 144-point launch took 20-30 ms instead of
   * 3), and six small pageable copies per launch cost more host time than the kernel of a small launch */
  if ((rc = ctx->h_eff.reserve(ctx, bytes, bytes / 2))) return rc;
  double *h_alpha = (double *)ctx->h_eff.p, *h_l = h_alpha + n;
  std::memcpy(h_alpha, alpha.data(), n * sizeof(double));
  std::memcpy(h_l, lcam.data(), n * sizeof(double));
  HIP_TRY(ctx, hipMemcpyAsync(d_alpha, h_alpha, 2 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  EscapeAngleParamsAdapt P;
  P.metric = MP;
  P.alpha = d_alpha;
  P.l_cam = d_l;
  P.angle = d_angle;
  P.space = d_space;
  P.steps = d_steps;
  P.status = d_status;
  P.n = (unsigned)n;
  P.max_iter = max_iter;
  P.max_radius = max_radius;
  P.delta = delta;
  P.fast_ok = cvk::metric_fast_ok(metric->kind, MP, max_radius) ? 1 : 0;
  P.kappa = kappa;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  with_kind(metric->kind, [&](auto K) {
    with_flag(ctx->fast_math != 0, [&](auto F) {
      constexpr int KIND = decltype(K)::value;
      constexpr bool FAST = decltype(F)::value;
      const dim3 grid((P.n + 63u) / 64u);
      if constexpr (FAST) /* option "step_scale": the fast step only (step_scale_kappa refuses the other) */
        if (adapt) {
          if (adapt == 2) hipLaunchKernelGGL((escape_angle_kernel<KIND, true, 2>), grid, dim3(64), 0, ctx->stream, P);
          else hipLaunchKernelGGL((escape_angle_kernel<KIND, true, 1>), grid, dim3(64), 0, ctx->stream, P);
          return;
        }
      hipLaunchKernelGGL((escape_angle_kernel<KIND, FAST>), grid, dim3(64), 0, ctx->stream, static_cast<const EscapeAngleParams &>(P));
    });
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  const size_t out_bytes = n * (2 * sizeof(double) + sizeof(unsigned) + sizeof(int));
  unsigned char *h_out = ctx->h_eff + 2 * n * sizeof(double);
  HIP_TRY(ctx, hipMemcpyAsync(h_out, d_angle, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(angle.data(), h_out, n * sizeof(double));
  std::memcpy(space.data(), h_out + n * sizeof(double), n * sizeof(double));
  std::memcpy(steps.data(), h_out + 2 * n * sizeof(double), n * sizeof(unsigned));
  std::memcpy(status.data(), h_out + 2 * n * sizeof(double) + n * sizeof(unsigned), n * sizeof(int));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (ms_acc) *ms_acc += ms;
  return CURVIS_OK;
}


/* The per-pixel kernel divides by four constants of the call -- the resolution (twice), pi and 2 pi -- and takes the first half of
 * those divisions, y = v_rcp_f64 + two Newton steps, from here: formed ONCE per context and resolution, on the device, by the same
 * instructions the compiler's own expansion of `/` uses (cv_device.h recip_chain), so that the kernel's quotients stay that expansion's
 * quotients bit for bit.  ~50 us, once. */
int ensure_pixel_recips(curvis_ctx *ctx, double res_x, double res_y, cvk::PixelRecips &out) {
  curvis_ctx::PixRecips &R = ctx->pix_recips;
  if (!R.valid || std::memcmp(&R.res_x, &res_x, sizeof res_x) != 0 || std::memcmp(&R.res_y, &res_y, sizeof res_y) != 0) {
    const double d[4] = {res_x, res_y, CV_PI, 2.0 * CV_PI};
    double y[4] = {0, 0, 0, 0};
    DeviceBuffer<double> dev; /* d | y */
    if (int rc = dev.reserve(ctx, 8)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dev, d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(recip_chain_kernel, dim3(1), dim3(64), 0, ctx->stream, dev.p, dev.p + 4, 4u);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(y, dev + 4, sizeof y, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; ++k) /* a resolution of 1 .. 2^32 and pi: nothing else can come out */
      if (!(y[k] > 0.0) || !std::isfinite(y[k])) return fail(ctx, CURVIS_E_HIP, "reciprocals of the pixel kernel's constants: not finite");
    R.res_x = res_x;
    R.res_y = res_y;
    R.y.y_res_x = y[0];
    R.y.y_res_y = y[1];
    R.y.y_pi = y[2];
    R.y.y_two_pi = y[3];
    R.valid = true;
  }
  out = R.y;
  return CURVIS_OK;
}

/* where the per-pixel kernel finds its inputs: offsets into this call's staging block (cameras, per-frame constants) and into the
 * block that holds the interpolation tables -- a sampler slot (device sampler) or the same staging block (host-paced sampler) */
struct PixelInputs {
  const unsigned char *call;
  size_t cams, frames;
  const unsigned char *tabs;
  size_t tab_off, tab_n, grid_off, grid, sx, m_e, c_e, m_s, c_s;
};
int make_pixel_params(curvis_ctx *ctx, uint32_t n_frames, uint32_t W, uint32_t H, const FrameCounters &FC, const PixelInputs &in,
                      EfficientPixelParams &Q) {
  for (int k = 0; k < 2; ++k) Q.sky[k] = make_sky_params(ctx, k);
  Q.cams = (const cvk::CameraParams *)(in.call + in.cams);
  Q.frames = (const cvk::EfficientFrame *)(in.call + in.frames);
  Q.tab_off = (const unsigned *)(in.tabs + in.tab_off);
  Q.tab_n = (const unsigned *)(in.tabs + in.tab_n);
  Q.grid_off = (const unsigned *)(in.tabs + in.grid_off);
  Q.grid = (const unsigned *)(in.tabs + in.grid);
  Q.sx = (const double *)(in.tabs + in.sx);
  Q.m_e = (const double *)(in.tabs + in.m_e);
  Q.c_e = (const double *)(in.tabs + in.c_e);
  Q.m_s = (const double *)(in.tabs + in.m_s);
  Q.c_s = (const double *)(in.tabs + in.c_s);
  Q.n_frames = n_frames;
  Q.W = W;
  Q.H = H;
  Q.fb = ctx->d_fb;
  Q.counters = FC;
  Q.w_magic = W > 1u ? ~0ull / W + 1ull : 0ull; /* floor((2^64 - 1) / W) + 1 = floor(2^64 / W) + 1 unless W divides 2^64, where it is 2^64 / W: exact too */
  return ensure_pixel_recips(ctx, (double)W, (double)H, Q.recips);
}

/* K3 over n_frames frames of Q.W x Q.H pixels: linear pixel order, or -- supersampled, or with option "sky_mipmap" (filter = 2), whose
 * quads need a lane's vertical neighbour in its wave -- 8x8 tiles of the fine grid, four per workgroup */
int launch_pixel_kernel(curvis_ctx *ctx, EfficientPixelParams Q, uint32_t n_frames, uint32_t ss, uint32_t filter, uint32_t projection) {
  Q.projection = (int)projection;
  const bool tiled = ss > 1u || filter == 2u || ctx->pixel_tiled != 0; /* "pixel_tiled": the enumeration alone, for measurements */
  const unsigned long long tiles = (unsigned long long)((Q.W + 7u) / 8u) * ((Q.H + 7u) / 8u);
  if (tiled && (tiles + 3ull) / 4ull > 0x7FFFFFFFull) return fail(ctx, CURVIS_E_INVALID, "frame or batch too large");
  const unsigned long long groups = tiled ? (tiles + 3ull) / 4ull : ((unsigned long long)Q.W * Q.H + 255ull) / 256ull;
  ctx->last_pixel_tiled = tiled ? 1 : 0;
  with_launch_shape(0, false, ss, filter, projection, false, [&](auto S) { /* the metric kind and the step flavour mean nothing to K3 */
    using T = decltype(S);
    const dim3 grid((unsigned)groups, n_frames);
    if constexpr (T::FILTER == 2) {
      WithSkyMip<EfficientPixelParams> QM;
      static_cast<EfficientPixelParams &>(QM) = Q;
      QM.mip = sky_mip_args(ctx);
      hipLaunchKernelGGL((efficient_pixel_ss_kernel<T::SS, 2, T::PROJ>), grid, dim3(256), 0, ctx->stream, QM);
    } else if constexpr (T::SS > 1) hipLaunchKernelGGL((efficient_pixel_ss_kernel<T::SS, T::FILTER, T::PROJ>), grid, dim3(256), 0, ctx->stream, Q);
    else if (tiled) hipLaunchKernelGGL((efficient_pixel_ss_kernel<1, T::FILTER, T::PROJ>), grid, dim3(256), 0, ctx->stream, Q);
    else hipLaunchKernelGGL((efficient_pixel_kernel<T::FILTER, T::PROJ>), grid, dim3(256), 0, ctx->stream, Q);
  });
  HIP_TRY(ctx, hipGetLastError());
  return CURVIS_OK;
}

/* per-frame and total statistics of an efficient render from the mirrored counters, the sampling and per-pixel kernel times and
 * the frames' sampling records (ctx->last_sampling_info, filled by whichever sampler ran) */
template <typename SampleMs> /* float: one HIP-event time (device sampler); double: a sum of them (host-paced) -- the quotients below keep that type */
void efficient_statistics(curvis_ctx *ctx, uint32_t n_frames, size_t npix, const FrameCounters &FC, SampleMs sample_ms, float pixel_ms,
                          curvis_stats *stats, std::chrono::steady_clock::time_point t_begin) {
  uint64_t tot[FC_N] = {0}, total_steps = 0;
  ctx->last_frame_stats.assign(n_frames, curvis_stats{});
  for (uint32_t f = 0; f < n_frames; ++f) {
    uint64_t fc[FC_N];
    sum_frame_counters(ctx->h_counters, FC.slots, f, fc);
    for (int k = 0; k < FC_N; ++k) tot[k] += fc[k];
    curvis_stats &fs = ctx->last_frame_stats[f];
    counts_to_stats(fc, fs);
    fs.rays = (uint64_t)npix; /* pixels; the integrator calls of the frame's sampler are in curvis_ctx_sampling_info */
    fs.steps = ctx->last_sampling_info[f].steps;
    total_steps += fs.steps;
    /* the samplers of a batch share their launches: times are the batch's, shared out evenly */
    fs.integrate_ms = sample_ms / n_frames;
    fs.shade_ms = pixel_ms / n_frames;
    fs.kernel_ms = fs.integrate_ms + fs.shade_ms;
    fs.total_ms = fs.kernel_ms;
  }
  if (stats) {
    counts_to_stats(tot, *stats);
    stats->rays = (uint64_t)npix * n_frames;
    stats->steps = total_steps;
    stats->integrate_ms = sample_ms;
    stats->shade_ms = pixel_ms;
    stats->kernel_ms = sample_ms + pixel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
}

/* ---- efficient mode with the DEVICE-RESIDENT sampler (kernels_efficient.h sampler_kernel) ------------------------------------
 * One launch samples every frame of the call -- a workgroup per distinct camera radius, rounds and all --, the per-pixel kernel
 * follows on the same stream and reads the tables where the sampler left them: no host round trip per refinement round, no
 * evaluation cache, no table building on the host.  What comes back is 32 bytes per job (counts and status) and the frame
 * counters; the sample tables themselves are fetched only if curvis_ctx_samples asks for them.
 * Returns CURVIS_OK, an error, or kSamplerFallback: a table outgrew the kernel's fixed arrays (cv_sampler_dev.h kSamplerCap) --
 * the caller then runs the host-paced sampler, which has no such bound. */
constexpr int kSamplerFallback = 1;

/* what a sampler launch depends on: two launches with equal keys produce equal tables */
curvis_ctx::SamplerKey make_sampler_key(const curvis_ctx *ctx, const EfficientCall &c) {
  curvis_ctx::SamplerKey k;
  k.metric = *c.metric;
  k.n_frames = c.n_frames;
  k.max_iter = c.max_iter;
  k.alpha_nums = c.alpha_nums;
  k.max_iterations_sampling = c.max_iterations_sampling;
  k.max_radius = c.max_radius, k.delta = c.delta, k.thr1 = c.thr1, k.thr2 = c.thr2;
  k.fast = ctx->fast_math != 0 ? 1 : 0;
  k.speculate = ctx->sampling_speculation != 0 ? 1 : 0; /* option "sampling_speculation" = 0 switches it off in the kernel too */
  k.step_scale = c.adapt ? ctx->step_scale : 0; /* a prefetch made under another value is another job: it is not consumed */
  k.integrator = c.adapt == 2 ? 1 : 0;          /* likewise */
  k.l_frame.resize(c.n_frames);
  for (uint32_t f = 0; f < c.n_frames; ++f) k.l_frame[f] = c.cams[f].pos[1];
  return k;
}
bool sampler_key_equal(const curvis_ctx::SamplerKey &a, const curvis_ctx::SamplerKey &b) {
  /* (field by field: the structs have padding, and a copy need not carry it; doubles by bit pattern) */
  auto same = [](const double &x, const double &y) { return std::memcmp(&x, &y, sizeof(double)) == 0; };
  if (a.metric.kind != b.metric.kind || !same(a.metric.rho, b.metric.rho) || !same(a.metric.m, b.metric.m) || !same(a.metric.a, b.metric.a))
    return false;
  if (a.n_frames != b.n_frames || a.max_iter != b.max_iter || a.alpha_nums != b.alpha_nums ||
      a.max_iterations_sampling != b.max_iterations_sampling || a.fast != b.fast || a.speculate != b.speculate || a.step_scale != b.step_scale ||
      a.integrator != b.integrator)
    return false;
  if (!same(a.max_radius, b.max_radius) || !same(a.delta, b.delta) || !same(a.thr1, b.thr1) || !same(a.thr2, b.thr2)) return false;
  return a.l_frame.size() == b.l_frame.size() &&
         std::memcmp(a.l_frame.data(), b.l_frame.data(), sizeof(double) * a.l_frame.size()) == 0;
}

/* Sample the frames of a call on `stream` into slot `slot` of the context (device buffer + page-locked mirror of its own): jobs,
 * staging, the sampler kernel, the jobs' results on their way back, an event when all of that is done.  Nothing waits here. */
int sampler_submit(curvis_ctx *ctx, unsigned slot, hipStream_t stream, const EfficientCall &c, const cvk::MetricParams &MP) {
  const curvis_camera *cams = c.cams;
  const uint32_t n_frames = c.n_frames;
  curvis_ctx::SamplerSlot &S = ctx->samp[slot];
  /* the slot's previous occupant may have been submitted on the OTHER stream (a prefetch nobody consumed, then a call that samples
   * itself, or the reverse): its kernel, its staging copy and its read-back must be over before the buffers are touched again.  It
   * was submitted two submissions ago, so this wait is over before it starts. */
  if (S.seq != 0 && S.done) HIP_TRY(ctx, hipEventSynchronize(S.done));
  if (ctx->dev_samples.valid && ctx->dev_samples.slot == slot) ctx->dev_samples.overwritten = true; /* curvis_ctx_samples: see fetch_device_samples */
  S.valid = false;
  /* jobs: one per distinct radial coordinate of the cameras (bit pattern) */
  S.job_of_frame.assign(n_frames, 0u);
  S.l_job.clear();
  {
    std::map<uint64_t, unsigned> seen;
    for (uint32_t f = 0; f < n_frames; ++f) {
      uint64_t key;
      std::memcpy(&key, &cams[f].pos[1], sizeof key);
      auto it = seen.find(key);
      if (it == seen.end()) {
        it = seen.emplace(key, (unsigned)S.l_job.size()).first;
        S.l_job.push_back(cams[f].pos[1]);
      }
      S.job_of_frame[f] = it->second;
    }
  }
  const unsigned n_jobs = (unsigned)S.l_job.size();
  const size_t T = (size_t)n_jobs * cvk::kSamplerCap, SS = (size_t)n_jobs * cvk::kSpecSlots;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  /* staged from the host in one copy ... */
  const size_t o_jf = carve(sizeof(unsigned) * n_frames), o_to = carve(sizeof(unsigned) * n_frames), o_go = carve(sizeof(unsigned) * n_frames),
               o_l = carve(sizeof(double) * n_jobs);
  const size_t staged = off;
  /* ... written by the sampler kernel */
  S.o_tab_off = o_to;
  S.o_grid_off = o_go;
  S.o_grid = carve(sizeof(unsigned) * n_jobs * (cvk::kInterpGrid + 1u));
  S.o_tab_n = carve(sizeof(unsigned) * n_frames);
  S.o_res = carve(sizeof(cvk::SamplerResult) * n_jobs);
  for (size_t &o : S.o_tab) o = carve(sizeof(double) * T);
  /* the jobs' evaluation caches (cv_sampler_dev.h SpecTable): 256 KB each */
  const size_t o_sk = carve(sizeof(unsigned long long) * SS), o_se = carve(sizeof(double) * SS), o_ss = carve(sizeof(double) * SS),
               o_st = carve(sizeof(unsigned) * SS), o_su = carve(sizeof(int) * SS);
  int rc = S.d.reserve(ctx, off);
  if (rc) return rc;
  S.res_bytes = sizeof(cvk::SamplerResult) * n_jobs;
  S.h_res_off = staged;
  const size_t pinned = staged + ((S.res_bytes + 255) & ~(size_t)255);
  if ((rc = S.h.reserve(ctx, pinned, pinned / 2))) return rc;
  if ((rc = S.done.ensure(ctx, hipEventDisableTiming))) return rc;
  if ((rc = S.t0.ensure(ctx))) return rc;
  if ((rc = S.t1.ensure(ctx))) return rc;
  std::memcpy(S.h + o_jf, S.job_of_frame.data(), sizeof(unsigned) * n_frames);
  {
    auto *to = reinterpret_cast<unsigned *>(S.h + o_to);
    auto *go = reinterpret_cast<unsigned *>(S.h + o_go);
    for (uint32_t f = 0; f < n_frames; ++f) {
      to[f] = S.job_of_frame[f] * cvk::kSamplerCap;
      go[f] = S.job_of_frame[f] * (cvk::kInterpGrid + 1u);
    }
  }
  std::memcpy(S.h + o_l, S.l_job.data(), sizeof(double) * n_jobs);
  HIP_TRY(ctx, hipMemcpyAsync(S.d, S.h, staged, hipMemcpyHostToDevice, stream));
  HIP_TRY(ctx, hipMemsetAsync(S.d + o_sk, 0xFF, sizeof(unsigned long long) * SS, stream)); /* every key = kSpecEmpty */
  curvis_ctx::SamplerKey key = make_sampler_key(ctx, c);
  SamplerParamsAdapt SP;
  SP.metric = MP;
  SP.l_cam = (const double *)(S.d + o_l);
  SP.n_jobs = n_jobs;
  SP.n_frames = n_frames;
  SP.job_of_frame = (const unsigned *)(S.d + o_jf);
  SP.tab_n = (unsigned *)(S.d + S.o_tab_n);
  SP.n0 = c.alpha_nums;
  SP.max_iterations = c.max_iterations_sampling;
  SP.max_iter = c.max_iter;
  SP.a_min = -0.1 * CV_PI; /* src/systems.rs:437-438 */
  SP.a_max = 1.1 * CV_PI;
  SP.thr1 = c.thr1;
  SP.thr2 = c.thr2;
  SP.max_radius = c.max_radius;
  SP.delta = c.delta;
  SP.fast_ok = cvk::metric_fast_ok(c.metric->kind, MP, c.max_radius) ? 1 : 0;
  SP.sx = (double *)(S.d + S.o_tab[0]);
  SP.se = (double *)(S.d + S.o_tab[1]);
  SP.ss = (double *)(S.d + S.o_tab[2]);
  SP.m_e = (double *)(S.d + S.o_tab[3]);
  SP.c_e = (double *)(S.d + S.o_tab[4]);
  SP.m_s = (double *)(S.d + S.o_tab[5]);
  SP.c_s = (double *)(S.d + S.o_tab[6]);
  SP.grid = (unsigned *)(S.d + S.o_grid);
  SP.res = (cvk::SamplerResult *)(S.d + S.o_res);
  SP.spec_key = (unsigned long long *)(S.d + o_sk);
  SP.spec_e = (double *)(S.d + o_se);
  SP.spec_s = (double *)(S.d + o_ss);
  SP.spec_steps = (unsigned *)(S.d + o_st);
  SP.spec_status = (int *)(S.d + o_su);
  SP.speculate = key.speculate;
  SP.kappa = c.kappa;
  HIP_TRY(ctx, hipEventRecord(S.t0, stream));
  with_kind(c.metric->kind, [&](auto K) {
    with_flag(key.fast != 0, [&](auto F) {
      constexpr int KIND = decltype(K)::value;
      constexpr bool FAST = decltype(F)::value;
      if constexpr (FAST) /* option "step_scale": the fast step only */
        if (c.adapt) {
          if (c.adapt == 2) hipLaunchKernelGGL((sampler_kernel<KIND, true, 2>), dim3(SP.n_jobs), dim3(kSamplerThreads), 0, stream, SP);
          else hipLaunchKernelGGL((sampler_kernel<KIND, true, 1>), dim3(SP.n_jobs), dim3(kSamplerThreads), 0, stream, SP);
          return;
        }
      hipLaunchKernelGGL((sampler_kernel<KIND, FAST>), dim3(SP.n_jobs), dim3(kSamplerThreads), 0, stream, static_cast<const SamplerParams &>(SP));
    });
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(S.t1, stream));
  HIP_TRY(ctx, hipMemcpyAsync(S.h + S.h_res_off, S.d + S.o_res, S.res_bytes, hipMemcpyDeviceToHost, stream));
  HIP_TRY(ctx, hipEventRecord(S.done, stream));
  S.key = std::move(key);
  S.seq = ++ctx->samp_seq;
  S.valid = true;
  return CURVIS_OK;
}

/* curvis_ctx_prefetch_efficient: the sampler of a FUTURE curvis_render_efficient_batch call, launched now on a stream of its own.
 * The sampler's cost is latency (a handful of Euler chains on a few compute units), the per-pixel kernel's and the PNG front end's
 * is throughput, and between them a render call leaves the GPU to the host (stream download, hand-over): the next call's sampler
 * fits into all of that.  The call with the same metric, settings and camera radii then waits for the event instead of sampling. */
int prefetch_efficient_impl(curvis_ctx *ctx, const EfficientCall &call) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!call.metric || !call.cams || call.n_frames == 0) return fail(ctx, CURVIS_E_INVALID, "null metric/camera or zero frames");
  EfficientCall c = call;
  if (int rc = step_scale_kappa(ctx, c.delta, c.kappa, c.adapt)) return rc; /* options "step_scale" and "integrator": part of what the job is */
  int rc = curvis_metric_validate(c.metric);
  if (rc != CURVIS_OK) return fail(ctx, rc, "invalid metric parameters (src/metrics.rs:409-456)");
  /* not a case for the device sampler, or (alpha_nums < 3) one that at most runs one round: the render call samples itself */
  if (c.alpha_nums < 3 || c.alpha_nums > cvk::kSamplerCap || c.alpha_nums > cvk::kSamplerPendCap) return CURVIS_OK;
  if (!(ctx->device_sampler > 0 || (ctx->device_sampler < 0 && c.n_frames >= (uint32_t)ctx->device_sampler_min_frames)))
    return CURVIS_OK; /* the render call will take the host-paced sampler: nothing to run ahead */
  for (uint32_t f = 0; f < c.n_frames; ++f)
    if (std::fabs(c.cams[f].pos[1]) > c.max_radius) return CURVIS_OK; /* the render call will report it */
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = ctx->sampler_stream.ensure(ctx, hipStreamNonBlocking))) return rc;
  const unsigned slot = ctx->samp_next;
  rc = sampler_submit(ctx, slot, ctx->sampler_stream, c, make_metric(*c.metric));
  if (rc) return rc;
  ctx->samp[slot].prefetched = true;
  ctx->samp_next = slot ^ 1u;
  ctx->prefetches++;
  return CURVIS_OK;
}

/* the tables of a call: prefetched by curvis_ctx_prefetch_efficient (either slot may hold them: ctx->stream then waits for that
 * slot's event), or sampled now on this call's stream.  The slot is consumed; its tables stay readable until it is submitted to again. */
int acquire_sampler_slot(curvis_ctx *ctx, const EfficientCall &c, const cvk::MetricParams &MP, int &slot, bool &prefetched) {
  const curvis_ctx::SamplerKey key = make_sampler_key(ctx, c);
  slot = -1;
  for (unsigned k = 0; k < 2u; ++k) /* both may match (every batch of an orbit has the same radii): the one submitted FIRST is the finished one */
    if (ctx->samp[k].valid && ctx->samp[k].prefetched && sampler_key_equal(ctx->samp[k].key, key) &&
        (slot < 0 || ctx->samp[k].seq < ctx->samp[slot].seq))
      slot = (int)k;
  prefetched = slot >= 0;
  if (!prefetched) {
    slot = (int)ctx->samp_next;
    const int rc = sampler_submit(ctx, (unsigned)slot, ctx->stream, c, MP);
    if (rc) return rc;
    ctx->samp_next = (unsigned)slot ^ 1u;
  } else {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->samp[slot].done, 0));
    ctx->prefetch_hits++;
  }
  ctx->samp[slot].prefetched = false;
  return CURVIS_OK;
}

/* what the device sampler's jobs report -> the context's sampling records of the last call */
void record_device_sampling(curvis_ctx *ctx, const curvis_ctx::SamplerSlot &S, const cvk::SamplerResult *h_res, uint32_t n_frames,
                            unsigned slot, bool prefetched, bool panic) {
  ctx->last_sampling_launches = 1;
  ctx->last_sampling_prefetched = prefetched ? 1 : 0;
  ctx->last_samples.assign(n_frames, {});
  ctx->last_sampling_info.assign(n_frames, curvis_sampling_info{});
  for (uint32_t f = 0; f < n_frames; ++f) {
    const cvk::SamplerResult &r = h_res[S.job_of_frame[f]];
    curvis_sampling_info &si = ctx->last_sampling_info[f];
    si.n_samples = r.n;
    si.rounds = r.rounds;
    si.calls = r.calls; /* what the reference's sampler of THIS frame calls and steps, whether or not frames shared the work */
    si.steps = r.steps;
    si.warned_max_iterations = r.warned;
  }
  uint64_t evaluated = 0;
  uint32_t chains = 0;
  for (size_t j = 0; j < S.l_job.size(); ++j) {
    evaluated += h_res[j].evaluated;
    chains = std::max(chains, h_res[j].eval_phases);
  }
  ctx->last_sampling_evaluated = evaluated;
  ctx->last_sampling_chains = chains; /* Euler chains the slowest job waited for: what the launch's latency is made of */
  ctx->dev_samples.valid = !panic;
  ctx->dev_samples.overwritten = false;
  ctx->dev_samples.slot = slot;
}

int render_efficient_device(curvis_ctx *ctx, const EfficientCall &c, const cvk::MetricParams &MP, const std::vector<cvk::EfficientFrame> &eframes,
                            uint8_t *rgb_out, curvis_stats *stats, std::chrono::steady_clock::time_point t_begin) {
  const uint32_t n_frames = c.n_frames, W = c.cams[0].res_x, H = c.cams[0].res_y;
  const size_t npix = (size_t)W * H;
  if (npix > 0xFFFFFFFFull || n_frames > 65535u) return fail(ctx, CURVIS_E_INVALID, "frame or batch too large");
  int slot = -1;
  bool prefetched = false;
  int rc = acquire_sampler_slot(ctx, c, MP, slot, prefetched);
  if (rc) return rc;
  curvis_ctx::SamplerSlot &S = ctx->samp[slot];
  const unsigned n_jobs = (unsigned)S.l_job.size();
  /* this call's own staging: cameras and per-frame constants */
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_cams = carve(staged_cameras_bytes(n_frames, c.boost)), o_fr = carve(sizeof(cvk::EfficientFrame) * n_frames);
  if ((rc = ctx->d_eff.reserve(ctx, off))) return rc;
  if ((rc = ctx->h_eff.reserve(ctx, off, off / 2))) return rc;
  unsigned char *stage = ctx->h_eff;
  {
    stage_cameras(stage + o_cams, c.cams, n_frames, c.boost);
    std::memcpy(stage + o_fr, eframes.data(), sizeof(cvk::EfficientFrame) * n_frames);
  }
  const size_t fb_bytes = (size_t)(W / c.ss) * (H / c.ss) * 3 * n_frames; /* W x H: the (fine) pixel grid; frames are W/ss x H/ss */
  rc = fb_begin_write(ctx, fb_bytes);
  if (rc) return rc;
  ctx->fb_bytes = fb_bytes;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_eff, stage, off, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  FrameCounters FC;
  rc = prepare_counters(ctx, n_frames, FC, 64u);
  if (rc) return rc;
  const size_t cnt_words = counter_words(n_frames, FC.slots);
  EfficientPixelParams Q;
  const PixelInputs in = {ctx->d_eff, o_cams, o_fr, S.d, S.o_tab_off, S.o_tab_n, S.o_grid_off, S.o_grid, S.o_tab[0], S.o_tab[3],
                          S.o_tab[4], S.o_tab[5], S.o_tab[6]};
  if ((rc = make_pixel_params(ctx, n_frames, W, H, FC, in, Q))) return rc;
  if ((rc = launch_pixel_kernel(ctx, Q, n_frames, c.ss, c.filter, c.projection))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(unsigned long long) * cnt_words, hipMemcpyDeviceToHost, ctx->stream));
  const auto t_launched = std::chrono::steady_clock::now();
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* (behind the sampler's event: its results are in S.h) */
  if (getenv("CURVIS_DEBUG_TIMING")) {
    float k_ms = 0.f;
    (void)hipEventElapsedTime(&k_ms, ctx->ev1, ctx->ev2);
    const auto t_now = std::chrono::steady_clock::now();
    fprintf(stderr, "[curvis] efficient call, %u frames (ms): host before the sync %.3f, in the sync %.3f (staging copy -> end of the per-pixel kernel: %.3f)\n",
            n_frames, std::chrono::duration<double, std::milli>(t_launched - t_begin).count(),
            std::chrono::duration<double, std::milli>(t_now - t_launched).count(), k_ms);
  }
  auto *h_res = reinterpret_cast<const cvk::SamplerResult *>(S.h + S.h_res_off);
  bool overflow = false, panic = false;
  for (unsigned j = 0; j < n_jobs; ++j) {
    overflow = overflow || h_res[j].status == cvk::SAMPLER_OVERFLOW;
    panic = panic || h_res[j].status == cvk::SAMPLER_PANIC;
  }
  if (getenv("CURVIS_DEBUG_TIMING"))
    for (unsigned j = 0; j < n_jobs; ++j)
      fprintf(stderr, "[curvis] device sampler job %u: l = %.17g -> %u samples, %u rounds, %llu calls, %llu steps, warned %d, status %d; "
              "%u Euler chains, %u points integrated%s\n", j, S.l_job[j], h_res[j].n, h_res[j].rounds, (unsigned long long)h_res[j].calls,
              (unsigned long long)h_res[j].steps, h_res[j].warned, h_res[j].status, h_res[j].eval_phases, h_res[j].evaluated,
              prefetched ? " (prefetched)" : "");
  if (overflow) return kSamplerFallback;
  float sample_ms = 0.f, ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&sample_ms, S.t0, S.t1)); /* the sampler kernel, wherever and whenever it ran */
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev1, ctx->ev2));
  record_device_sampling(ctx, S, h_res, n_frames, (unsigned)slot, prefetched, panic);
  if (panic)
    return fail(ctx, CURVIS_E_SAMPLING,
                "sampler panic: fewer than 3 finite samples (src/sampling.rs:155-157) or undefined tangent rotation "
                "(src/algebra.rs:95-97)");
  if (rgb_out) {
    rc = fb_download(ctx, rgb_out, fb_bytes);
    if (rc) return rc;
  }
  efficient_statistics(ctx, n_frames, npix, FC, sample_ms, ms, stats, t_begin);
  return CURVIS_OK;
}

/* the sample table of frame `frame` of the last render_efficient call that used the device-resident sampler: fetched from the
 * context's scratch on demand (curvis_ctx_samples), once per frame asked for */
int fetch_device_samples(curvis_ctx *ctx, uint32_t frame) {
  if (!ctx->dev_samples.valid) return CURVIS_OK;
  const curvis_ctx::SamplerSlot &S = ctx->samp[ctx->dev_samples.slot];
  if (frame >= S.job_of_frame.size() || frame >= ctx->last_samples.size()) return CURVIS_OK;
  if (!ctx->last_samples[frame].empty() || ctx->last_sampling_info[frame].n_samples == 0) return CURVIS_OK;
  if (ctx->dev_samples.overwritten)
    return fail(ctx, CURVIS_E_INVALID, "the sample tables of that render call are gone: a later curvis_ctx_prefetch_efficient has taken their slot "
                                       "(ask for them before the second prefetch after the call)");
  const size_t n = ctx->last_sampling_info[frame].n_samples, o = (size_t)S.job_of_frame[frame] * cvk::kSamplerCap * sizeof(double);
  std::vector<double> a(n), e(n), s(n);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpy(a.data(), S.d + S.o_tab[0] + o, n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(e.data(), S.d + S.o_tab[1] + o, n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(s.data(), S.d + S.o_tab[2] + o, n * sizeof(double), hipMemcpyDeviceToHost));
  auto &pts = ctx->last_samples[frame];
  pts.resize(n);
  for (size_t i = 0; i < n; ++i) pts[i] = cvs::BiPoint{a[i], e[i], s[i]};
  return CURVIS_OK;
}

/* ---- efficient mode with the HOST-PACED sampler (cv_sampler.h): one sampler per frame, advanced in lock step; every round is ONE
 * kernel launch.  It has no bound on the table size, and it is the device sampler's checker. */

/* Evaluation cache + speculation.  Every point the sampler will ever ask for is the midpoint of two
 * samples that are adjacent at that time, i.e. a node of the dyadic tree below an interval of the current
 * table, computed by the same (lo + hi) / 2.0.  So whenever some requested alpha is not cached yet, the
 * launch also evaluates the whole subtree of depth `spec` below the interval it comes from (and, on the
 * first launch, below every interval of the uniform grid): the GPU is idle anyway -- a round is a single
 * wave's 2000-step dependency chain -- and the following rounds are then served from the cache without
 * a launch.  The sampler consumes exactly the values the sequential algorithm would compute; calls and
 * steps are counted at consumption, so the bookkeeping equals the reference's. */
/* open-addressing table keyed by the bit pattern of alpha; state 0 = empty, 1 = queued for the next launch,
 * 2 = evaluated (a node-based std::unordered_map cost more host time per batch than the kernels) */
struct Cached {
  uint64_t key;
  double e, s;
  uint32_t steps;
  int status;
  uint32_t state;
};
struct EvalCache {
  std::vector<Cached> slots;
  size_t used = 0;
  explicit EvalCache(size_t capacity = 4096) : slots(capacity, Cached{0, 0.0, 0.0, 0, 0, 0}) {}
  static size_t hash(uint64_t k) { return (size_t)((k * 0x9E3779B97F4A7C15ull) >> 20); }
  Cached *find(uint64_t k) { /* the slot holding k, or the empty slot where it would go */
    const size_t mask = slots.size() - 1;
    size_t i = hash(k) & mask;
    while (slots[i].state != 0 && slots[i].key != k) i = (i + 1) & mask;
    return &slots[i];
  }
  Cached *claim(uint64_t k) { /* find, inserting an empty (state 0) entry for a new key */
    if (2 * (used + 1) > slots.size()) {
      std::vector<Cached> old;
      old.swap(slots);
      slots.assign(old.size() * 2, Cached{0, 0.0, 0.0, 0, 0, 0});
      for (const Cached &c : old)
        if (c.state != 0) *find(c.key) = c;
    }
    Cached *c = find(k);
    if (c->state == 0) c->key = k;
    return c;
  }
};
inline uint64_t key_of(double a) {
  uint64_t u;
  std::memcpy(&u, &a, sizeof u);
  return u;
}

/* step 3 on the host: drives smp[f] (one per frame, set up by the caller) to the end; counts launches and evaluated points into the
 * context, adds the kernels' time to sample_ms, and reports a panic of the integrator (the samplers report their own) */
int sample_host_paced(curvis_ctx *ctx, const EfficientCall &c, const cvk::MetricParams &MP, std::vector<cvs::Sampler> &smp, double &sample_ms,
                      bool &panic) {
  const uint32_t n_frames = c.n_frames, alpha_nums = c.alpha_nums;
  const curvis_camera *cams = c.cams;
  int rc;
  /* automatic depths: about 30-50 k points per launch (tools/gpu_eff_two_launch.py, tools/gpu_eff_batch_spec.py) */
  const int spec = ctx->sampling_speculation < 0 ? (n_frames <= 2 ? 10 : n_frames <= 5 ? 6 : 4)
                                                 : (ctx->sampling_speculation > 11 ? 11 : ctx->sampling_speculation);
  /* depth of the subtrees evaluated below the intervals of the initial uniform grid (first launch) */
  const int first_cap = ctx->sampling_speculation_first < 0 ? (n_frames <= 2 ? 8 : n_frames <= 5 ? 4 : 3)
                                                            : (ctx->sampling_speculation_first > 11 ? 11 : ctx->sampling_speculation_first);
  /* sized for the first launch (grid x subtree) plus as much again, so that the table is not rebuilt four times on
   * the way up from a small default (a quarter of the host time of a single image) */
  size_t cache_cap = 4096;
  {
    const size_t first = (size_t)alpha_nums << (spec > 0 ? (spec > first_cap ? first_cap : spec) : 0);
    while (cache_cap < 4 * first && cache_cap < ((size_t)1 << 22)) cache_cap *= 2;
  }
  std::vector<EvalCache> cache;
  cache.reserve(n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) cache.emplace_back(cache_cap);
  std::vector<char> planned(n_frames, 0);
  uint64_t evaluated = 0;
  uint32_t launches = 0;
  std::vector<double> b_alpha, b_l, r_angle, r_space, ce, cs;
  std::vector<uint32_t> r_steps, cst;
  std::vector<int> r_status;
  std::vector<uint32_t> b_frame;
  const bool dbg_timing = getenv("CURVIS_DEBUG_TIMING") != nullptr;
  double t_adv = 0.0, t_build = 0.0, t_eval = 0.0, t_ins = 0.0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  for (;;) {
    const auto tp0 = now();
    /* advance every sampler as far as the cache allows */
    bool any_waiting = false;
    for (uint32_t f = 0; f < n_frames; ++f) {
      for (;;) {
        if (!planned[f]) {
          if (!smp[f].plan()) break; /* finished */
          planned[f] = 1;
        }
        bool all_cached = true;
        for (double a : smp[f].pending)
          if (cache[f].find(key_of(a))->state != 2) {
            all_cached = false;
            break;
          }
        if (!all_cached) {
          any_waiting = true;
          break;
        }
        const size_t n = smp[f].pending.size();
        ce.resize(n);
        cs.resize(n);
        cst.resize(n);
        for (size_t k = 0; k < n; ++k) {
          const Cached &c = *cache[f].find(key_of(smp[f].pending[k]));
          ce[k] = c.e;
          cs[k] = c.s;
          cst[k] = c.steps;
          if (c.status == cvk::ESC_PANIC) panic = true;
        }
        smp[f].consume(ce.data(), cs.data(), cst.data());
        planned[f] = 0;
      }
    }
    const auto tp1 = now();
    t_adv += secs(tp0, tp1);
    if (!any_waiting) break;
    /* one launch: the missing points of every waiting frame plus their speculative subtrees */
    b_alpha.clear();
    b_l.clear();
    b_frame.clear();
    for (uint32_t f = 0; f < n_frames; ++f) {
      if (!planned[f]) continue;
      auto want = [&](double a) {
        Cached *c = cache[f].claim(key_of(a));
        if (c->state != 0) return; /* evaluated, or already queued for this launch */
        c->state = 1;
        cache[f].used++;
        b_alpha.push_back(a);
        b_l.push_back(cams[f].pos[1]);
        b_frame.push_back(f);
      };
      struct Node {
        double lo, hi;
        int depth;
      };
      std::vector<Node> stack;
      const cvs::Sampler &S = smp[f];
      for (size_t k = 0; k < S.pending.size(); ++k) {
        want(S.pending[k]);
        if (spec <= 0) continue;
        if (S.pend_lo[k] == S.pend_lo[k]) {
          stack.push_back(Node{S.pend_lo[k], S.pend_hi[k], spec});
        } else if (k + 1 < S.pending.size()) { /* uniform grid: subtree below [x_k, x_{k+1}] */
          stack.push_back(Node{S.pending[k], S.pending[k + 1], spec > first_cap ? first_cap : spec});
        }
        while (!stack.empty()) {
          const Node nd = stack.back();
          stack.pop_back();
          const double mid = (nd.lo + nd.hi) / 2.0;
          if (!(mid > nd.lo && mid < nd.hi)) continue; /* interval exhausted in double precision */
          want(mid);
          if (nd.depth > 1) {
            stack.push_back(Node{nd.lo, mid, nd.depth - 1});
            stack.push_back(Node{mid, nd.hi, nd.depth - 1});
          }
        }
      }
    }
    const auto tp2 = now();
    t_build += secs(tp1, tp2);
    rc = eval_escape_batch(ctx, c.metric, MP, b_alpha, b_l, c.max_iter, c.max_radius, c.delta, r_angle, r_space, r_steps, r_status, &sample_ms, c.adapt, c.kappa);
    if (rc) return rc;
    const auto tp3 = now();
    t_eval += secs(tp2, tp3);
    ++launches;
    evaluated += b_alpha.size();
    for (size_t k = 0; k < b_alpha.size(); ++k) {
      Cached *c = cache[b_frame[k]].find(key_of(b_alpha[k]));
      c->e = r_angle[k];
      c->s = r_space[k];
      c->steps = r_steps[k];
      c->status = r_status[k];
      c->state = 2;
    }
    t_ins += secs(tp3, now());
  }
  if (dbg_timing)
    fprintf(stderr, "[curvis] sampling host phases (ms): advance %.3f, build %.3f, evaluate (copies+kernel+sync) %.3f of which kernels %.3f, cache insert %.3f; launches %u, points %llu\n",
            t_adv, t_build, t_eval, sample_ms, t_ins, launches, (unsigned long long)evaluated);
  ctx->last_sampling_launches = launches;
  ctx->last_sampling_evaluated = evaluated;
  return CURVIS_OK;
}

/* the finished samplers -> the context's sampling records of the last call; true if one of them panicked */
bool record_host_sampling(curvis_ctx *ctx, const std::vector<cvs::Sampler> &smp) {
  const uint32_t n_frames = (uint32_t)smp.size();
  bool panic = false;
  ctx->last_samples.assign(n_frames, {});
  ctx->last_sampling_info.assign(n_frames, curvis_sampling_info{});
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (smp[f].panicked) panic = true;
    ctx->last_samples[f] = smp[f].pts;
    curvis_sampling_info &si = ctx->last_sampling_info[f];
    si.n_samples = (uint32_t)smp[f].pts.size();
    si.rounds = smp[f].rounds;
    si.calls = smp[f].calls;
    si.steps = smp[f].steps;
    si.warned_max_iterations = smp[f].warned ? 1 : 0;
  }
  return panic;
}

/* step 4 tables (interp 1.0.3) of every frame, back to back; a frame with an empty table still takes one slot */
struct InterpTables {
  std::vector<double> sx, m_e, c_e, m_s, c_s;
  std::vector<unsigned> tab_off, tab_n, grid_off, grid; /* grid: cv_efficient.h interp_index_grid */
};
InterpTables build_interp_tables(const std::vector<cvs::Sampler> &smp) {
  const uint32_t n_frames = (uint32_t)smp.size();
  InterpTables t;
  std::vector<double> &sx = t.sx, &m_e = t.m_e, &c_e = t.c_e, &m_s = t.m_s, &c_s = t.c_s, x, ye, ys, m, c;
  std::vector<unsigned> &tab_off = t.tab_off, &tab_n = t.tab_n, &grid_off = t.grid_off, &grid = t.grid;
  tab_off.resize(n_frames), tab_n.resize(n_frames), grid_off.resize(n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    const auto &pts = smp[f].pts;
    x.clear();
    ye.clear();
    ys.clear();
    for (const auto &b : pts) {
      x.push_back(b.a);
      ye.push_back(b.e);
      ys.push_back(b.s);
    }
    tab_off[f] = (unsigned)sx.size();
    tab_n[f] = (unsigned)pts.size();
    const size_t slots = std::max<size_t>(pts.size(), 1);
    cvs::interp_tables(x, ye, m, c);
    m.resize(slots, 0.0);
    c.resize(slots, 0.0);
    m_e.insert(m_e.end(), m.begin(), m.end());
    c_e.insert(c_e.end(), c.begin(), c.end());
    cvs::interp_tables(x, ys, m, c);
    m.resize(slots, 0.0);
    c.resize(slots, 0.0);
    m_s.insert(m_s.end(), m.begin(), m.end());
    c_s.insert(c_s.end(), c.begin(), c.end());
    grid_off[f] = (unsigned)grid.size();
    grid.resize(grid.size() + cvk::kInterpGrid + 1u, 0u);
    for (unsigned i = 0; i <= (unsigned)pts.size(); ++i) cvk::interp_grid_fill(x.data(), (unsigned)pts.size(), i, grid.data() + grid_off[f]);
    x.resize(slots, 0.0);
    sx.insert(sx.end(), x.begin(), x.end());
  }
  return t;
}

/* K3 from host-built tables: one staging block (cameras, per-frame constants, tables), the per-pixel kernel, statistics */
int render_pixels_staged(curvis_ctx *ctx, const EfficientCall &c, const std::vector<cvk::EfficientFrame> &eframes, const InterpTables &t,
                         double sample_ms, uint8_t *rgb_out, curvis_stats *stats, std::chrono::steady_clock::time_point t_begin) {
  const uint32_t n_frames = c.n_frames, W = c.cams[0].res_x, H = c.cams[0].res_y;
  /* device buffers for K3 */
  const size_t npix = (size_t)W * H;
  if (npix > 0xFFFFFFFFull || n_frames > 65535u) return fail(ctx, CURVIS_E_INVALID, "frame or batch too large");
  const size_t fb_bytes = (size_t)(W / c.ss) * (H / c.ss) * 3 * n_frames; /* W x H: the (fine) pixel grid; frames are W/ss x H/ss */
  int rc = fb_begin_write(ctx, fb_bytes);
  if (rc) return rc;
  ctx->fb_bytes = fb_bytes;
  const size_t T = t.sx.size();
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 15) & ~(size_t)15;
    return o;
  };
  const size_t o_cams = carve(staged_cameras_bytes(n_frames, c.boost)), o_fr = carve(sizeof(cvk::EfficientFrame) * n_frames),
               o_to = carve(sizeof(unsigned) * n_frames), o_tn = carve(sizeof(unsigned) * n_frames),
               o_go = carve(sizeof(unsigned) * n_frames), o_gr = carve(sizeof(unsigned) * t.grid.size()),
               o_sx = carve(sizeof(double) * T), o_me = carve(sizeof(double) * T), o_ce = carve(sizeof(double) * T),
               o_ms = carve(sizeof(double) * T), o_cs = carve(sizeof(double) * T);
  if ((rc = ctx->d_eff.reserve(ctx, off))) return rc;
  std::vector<unsigned char> stage(off);
  stage_cameras(stage.data() + o_cams, c.cams, n_frames, c.boost);
  std::memcpy(stage.data() + o_fr, eframes.data(), sizeof(cvk::EfficientFrame) * n_frames);
  std::memcpy(stage.data() + o_to, t.tab_off.data(), sizeof(unsigned) * n_frames);
  std::memcpy(stage.data() + o_tn, t.tab_n.data(), sizeof(unsigned) * n_frames);
  std::memcpy(stage.data() + o_go, t.grid_off.data(), sizeof(unsigned) * n_frames);
  std::memcpy(stage.data() + o_gr, t.grid.data(), sizeof(unsigned) * t.grid.size());
  std::memcpy(stage.data() + o_sx, t.sx.data(), sizeof(double) * T);
  std::memcpy(stage.data() + o_me, t.m_e.data(), sizeof(double) * T);
  std::memcpy(stage.data() + o_ce, t.c_e.data(), sizeof(double) * T);
  std::memcpy(stage.data() + o_ms, t.m_s.data(), sizeof(double) * T);
  std::memcpy(stage.data() + o_cs, t.c_s.data(), sizeof(double) * T);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_eff, stage.data(), off, hipMemcpyHostToDevice, ctx->stream));
  FrameCounters FC;
  rc = prepare_counters(ctx, n_frames, FC, 64u); /* one workgroup in 256 pixels adds to them: spread over 64 lines per frame */
  if (rc) return rc;
  const size_t cnt_words = counter_words(n_frames, FC.slots);
  EfficientPixelParams Q;
  const PixelInputs in = {ctx->d_eff, o_cams, o_fr, ctx->d_eff, o_to, o_tn, o_go, o_gr, o_sx, o_me, o_ce, o_ms, o_cs};
  if ((rc = make_pixel_params(ctx, n_frames, W, H, FC, in, Q))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if ((rc = launch_pixel_kernel(ctx, Q, n_frames, c.ss, c.filter, c.projection))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(unsigned long long) * cnt_words,
                              hipMemcpyDeviceToHost, ctx->stream));
  if (rgb_out) {
    rc = fb_download(ctx, rgb_out, fb_bytes); /* leaves the stream idle; option "async_download": the frames follow */
    if (rc) return rc;
  } else {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  efficient_statistics(ctx, n_frames, npix, FC, sample_ms, ms, stats, t_begin);
  return CURVIS_OK;
}

int render_efficient_impl(curvis_ctx *ctx, const EfficientCall &call, uint8_t *rgb_out, curvis_stats *stats) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!call.metric || !call.cams || call.n_frames == 0) return fail(ctx, CURVIS_E_INVALID, "null metric/camera or zero frames");
  /* option "supersample" = N > 1: the call over the N times finer pixel grid (the samplers see camera radii only and do not notice),
   * averaged into res_x x res_y frames by the per-pixel kernel; "rays" are fine pixels;
   * option "sky_filter" = 1: the per-pixel kernel blends; the samplers never see a sky;
   * option "projection" != 0: the per-pixel kernel forms other directions; the samplers tabulate the whole sphere as it is */
  EfficientCall c = call;
  CallShape shape;
  if (int rc = prepare_call_shape(ctx, c.cams, c.n_frames, c.delta, "frame or batch too large", shape)) return rc;
  c.kappa = shape.kappa;
  c.adapt = shape.adapt;
  c.ss = shape.ss;
  c.filter = shape.filter;
  c.projection = shape.projection;
  c.boost = shape.boost.empty() ? nullptr : shape.boost.data();
  const curvis_metric *metric = c.metric;
  const curvis_camera *cams = c.cams;
  const uint32_t n_frames = c.n_frames, alpha_nums = c.alpha_nums;
  const double max_radius = c.max_radius;
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = curvis_metric_validate(metric);
  if (rc != CURVIS_OK) return fail(ctx, rc, "invalid metric parameters (src/metrics.rs:409-456)");
  if ((rc = schwarzschild_camera_check(ctx, metric, cams, n_frames))) return rc;
  const uint32_t W = cams[0].res_x, H = cams[0].res_y;
  if (W == 0 || H == 0) return fail(ctx, CURVIS_E_INVALID, "resolution must be greater than 0 (src/cameras.rs:98)");
  /* compute_uniform_range's `alpha_nums - 1` underflows for 0 (a panic in the reference's default build).  1 and 2 are NOT refused:
   * the reference panics only inside evaluate_denser_bipoints (src/sampling.rs:155-157), i.e. when a refinement round starts with
   * fewer than 3 finite samples -- both samplers raise CURVIS_E_SAMPLING there themselves --; with max_iterations_sampling = 0 it
   * returns a frame from a table of 0, 1 or 2 samples */
  if (alpha_nums == 0) return fail(ctx, CURVIS_E_SAMPLING, "alpha_nums == 0: compute_uniform_range underflows (src/sampling.rs:133)");
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (cams[f].res_x != W || cams[f].res_y != H)
      return fail(ctx, CURVIS_E_INVALID, "all cameras of a batch must share one resolution");
    if (std::fabs(cams[f].pos[1]) > max_radius)
      return fail(ctx, CURVIS_E_CAMERA_OUTSIDE,
                  "Photon already beyond the maximum radius. Cannot evaluate escape. (src/systems.rs:122-124)");
  }
  if (!ctx->sky[0].texels || !ctx->sky[1].texels) return fail(ctx, CURVIS_E_NO_SKY, "both background images must be set");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (c.filter == 2u) /* option "sky_mipmap": the skies' mip chains, built on first use, before anything of the call is timed */
    for (int k = 0; k < 2; ++k)
      if ((rc = ensure_sky_mips(ctx, k))) return rc;
  const cvk::MetricParams MP = make_metric(*metric);

  /* step 1 (host): camera direction on the background space and the tangent->background rotation */
  std::vector<cvk::EfficientFrame> eframes(n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (!cvk::efficient_frame_pose(cams[f].pos[2], cams[f].pos[3], eframes[f])) /* platform libm: cv_frame_host.h */
      return fail(ctx, CURVIS_E_PARALLEL, "v1 and v2 must not be parallel (src/algebra.rs:95-97, camera on the x axis)");
  }

  ctx->dev_samples.valid = false;
  /* step 3 on the device (sampler_kernel: no host in the refinement loop) for calls of `device_sampler_min_frames` frames and
   * more -- its latency is rounds x one Euler chain, about three times the speculating host-paced sampler's below, and what it
   * saves is host time and launches per frame, so single images and small batches stay on the host-paced path (cross-over measured
   * between 32 and 64 frames per call); option "device_sampler": 1 always, 0 never, -1 (default) by that threshold */
  const bool want_device = ctx->device_sampler > 0 || (ctx->device_sampler < 0 && n_frames >= (uint32_t)ctx->device_sampler_min_frames);
  if (want_device && alpha_nums <= cvk::kSamplerCap && alpha_nums <= cvk::kSamplerPendCap) {
    rc = render_efficient_device(ctx, c, MP, eframes, rgb_out, stats, t_begin);
    ctx->last_sampler_path = rc == kSamplerFallback ? 2 : 1;
    if (rc != kSamplerFallback) return rc;
    ctx->dev_samples.valid = false; /* a table outgrew the kernel's arrays: the host-paced sampler takes the call */
  } else {
    ctx->last_sampler_path = 0;
  }
  /* step 3 on the host: one sampler per frame, advanced in lock step; every round is ONE kernel launch */
  std::vector<cvs::Sampler> smp(n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    smp[f].a_min = -0.1 * CV_PI; /* src/systems.rs:437-438 */
    smp[f].a_max = 1.1 * CV_PI;
    smp[f].n0 = alpha_nums;
    smp[f].max_iterations = c.max_iterations_sampling;
    smp[f].thr1 = c.thr1;
    smp[f].thr2 = c.thr2;
  }
  double sample_ms = 0.0;
  bool panic = false;
  if ((rc = sample_host_paced(ctx, c, MP, smp, sample_ms, panic))) return rc;
  panic = record_host_sampling(ctx, smp) || panic;
  if (panic)
    return fail(ctx, CURVIS_E_SAMPLING,
                "sampler panic: fewer than 3 finite samples (src/sampling.rs:155-157) or undefined tangent rotation "
                "(src/algebra.rs:95-97)");

  return render_pixels_staged(ctx, c, eframes, build_interp_tables(smp), sample_ms, rgb_out, stats, t_begin);
}

int render_direct_impl(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cam, uint32_t max_iter,
                       double max_radius, double delta, uint8_t *rgb_out, curvis_stats *stats) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!metric || !cam) return fail(ctx, CURVIS_E_INVALID, "null metric/camera");
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = curvis_metric_validate(metric);
  if (rc != CURVIS_OK) return fail(ctx, rc, "invalid metric parameters (src/metrics.rs:409-456)");
  /* option "supersample" = N > 1: the camera of the N times finer grid, averaged into res_x x res_y by the kernel's epilogue */
  WithCameraBoost<DirectParamsAdapt> P; /* the widest argument: every form's is a base of it, or (FILTER = 2) built from one */
  CallShape shape;
  if ((rc = schwarzschild_camera_check(ctx, metric, cam, 1))) return rc;
  if ((rc = prepare_call_shape(ctx, cam, 1, delta, "frame too large", shape))) return rc;
  P.kappa = shape.kappa;
  const uint32_t ss = shape.ss, filter = shape.filter;
  P.projection = (int)shape.projection;
  P.boost = shape.boost.empty() ? cvk::CameraBoost{} : shape.boost[0];
  const uint32_t W = cam->res_x, H = cam->res_y;
  if (W == 0 || H == 0) return fail(ctx, CURVIS_E_INVALID, "resolution must be greater than 0 (src/cameras.rs:98)");
  if (std::fabs(cam->pos[1]) > max_radius)
    return fail(ctx, CURVIS_E_CAMERA_OUTSIDE, "Photon already beyond the maximum radius. Cannot evaluate escape. (src/systems.rs:122-124)");
  if (!ctx->sky[0].texels || !ctx->sky[1].texels) return fail(ctx, CURVIS_E_NO_SKY, "both background images must be set");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  P.metric = make_metric(*metric);
  P.cam = make_camera(*cam);
  if (!cvk::efficient_frame_pose(cam->pos[2], cam->pos[3], P.frame)) /* src/systems.rs:393-397, :411 */
    return fail(ctx, CURVIS_E_PARALLEL, "v1 and v2 must not be parallel (src/algebra.rs:95-97, camera on the x axis)");
  for (int k = 0; k < 2; ++k) P.sky[k] = make_sky_params(ctx, k);
  if (filter == 2u) /* option "sky_mipmap": the skies' mip chains, built on first use */
    for (int k = 0; k < 2; ++k)
      if ((rc = ensure_sky_mips(ctx, k))) return rc;
  P.W = W;
  P.H = H;
  P.tiles_x = (W + 7) / 8;
  P.tiles_y = (H + 7) / 8;
  P.total_rays = (unsigned long long)P.tiles_x * P.tiles_y * 64ull;
  if (P.total_rays / 64ull > 0xFFFFFFFFull) return fail(ctx, CURVIS_E_INVALID, "frame too large");
  P.max_iter = max_iter;
  P.max_radius = max_radius;
  P.delta = delta;
  P.fast_ok = cvk::metric_fast_ok(metric->kind, P.metric, max_radius) ? 1 : 0;
  const size_t fb_bytes = (size_t)(W / ss) * (H / ss) * 3;
  rc = fb_begin_write(ctx, fb_bytes);
  if (rc) return rc;
  ctx->fb_bytes = fb_bytes;
  P.fb = ctx->d_fb;
  FrameCounters FC;
  rc = prepare_counters(ctx, 1, FC);
  if (rc) return rc;
  P.counters = FC;
  const size_t cnt_words = counter_words(1, FC.slots);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  with_launch_shape(metric->kind, ctx->fast_math != 0, ss, filter, shape.projection, shape.adapt, [&](auto S) {
    using T = decltype(S);
    const dim3 grid((unsigned)((P.total_rays + 255ull) / 256ull));
    DirectArgs<T::ADAPT, T::FILTER, T::PROJ> A; /* the form's own argument: the boost behind PROJ = 1, the level tables behind FILTER = 2 */
    static_cast<std::conditional_t<T::ADAPT != 0, DirectParamsAdapt, DirectParams> &>(A) = P;
    if constexpr (T::PROJ != 0) A.boost = P.boost;
    if constexpr (T::FILTER == 2) {
      A.mip = sky_mip_args(ctx);
      hipLaunchKernelGGL((direct_kernel<T::KIND, T::FAST, T::SS, 2, T::PROJ, T::ADAPT>), grid, dim3(256), 0, ctx->stream, A);
    } else if constexpr (T::ADAPT != 0) hipLaunchKernelGGL((direct_kernel<T::KIND, T::FAST, T::SS, T::FILTER, T::PROJ, T::ADAPT>), grid, dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL((direct_kernel<T::KIND, T::FAST, T::SS, T::FILTER, T::PROJ>), grid, dim3(256), 0, ctx->stream, A);
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(unsigned long long) * cnt_words, hipMemcpyDeviceToHost, ctx->stream));
  if (rgb_out) {
    rc = fb_download(ctx, rgb_out, fb_bytes); /* leaves the stream idle; option "async_download": the frames follow */
    if (rc) return rc;
  } else {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  uint64_t fc[FC_N];
  sum_frame_counters(ctx->h_counters, FC.slots, 0, fc);
  curvis_stats st;
  std::memset(&st, 0, sizeof st);
  counts_to_stats(fc, st);
  st.kernel_ms = st.integrate_ms = ms;
  st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  ctx->last_frame_stats.assign(1, st);
  ctx->last_integrate_ms = ms;
  ctx->last_shade_ms = 0.0;
  ctx->last_relay_launches = 0;
  if (stats) *stats = st;
  return CURVIS_OK;
}

}  // namespace
