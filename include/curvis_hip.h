/* curvis_hip.h -- C ABI of libcurvis_hip.so: the MI355X (gfx950) replacement for the
 * per-pixel geodesic hot path of fragarriss/CurVis.
 *
 * The reference has no FFI/plugin seam; the seam this library replaces is the method pair its
 * orchestration calls (src/rendering.rs:97 and :299):
 *
 *   RelativisticSystem<M>::render_image(&self, max_iterations: u32, max_radius: f64, delta: f64)
 *        -> image::DynamicImage                                          src/systems.rs:307-330
 *   RelativisticSystem<M>::render_image_efficient(&self, max_iterations_propagation, max_radius, delta,
 *        alpha_nums, max_iterations_sampling, thr1, thr2) -> DynamicImage  src/systems.rs:333-527
 *
 * with self = { metric: M, background_positive, background_negative: SphericalImage, camera: Camera }
 * (src/systems.rs:68-73).  A context (`curvis_ctx`) plays the role of `self`: it owns one GPU, the
 * two sky textures resident in HBM, and the device framebuffer.  A Rust host binds these with a
 * plain `extern "C"` block (INTEGRATION.md shows the stub); the C++ host in curvis_amd/csrc/host and
 * the Python mirror in curvis_amd/ bind the same symbols.
 *
 * Conventions: every function returns CURVIS_OK (0) or a negative CURVIS_E_* code;
 * curvis_last_error() gives the message.  The reference's panics map to error codes.  A context is
 * not thread-safe; distinct contexts (one per GPU) are independent.  No CPU fallback exists: without
 * a gfx950 device curvis_ctx_create fails with CURVIS_E_NO_DEVICE.
 */
#ifndef CURVIS_HIP_H
#define CURVIS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CURVIS_ABI_VERSION 1

enum {
  CURVIS_OK = 0,
  CURVIS_E_INVALID = -1,        /* bad argument (null pointer, zero resolution, ...) */
  CURVIS_E_NO_DEVICE = -2,      /* no usable gfx950 GPU: the product path has no CPU fallback */
  CURVIS_E_HIP = -3,            /* a HIP runtime call failed */
  CURVIS_E_CAMERA_OUTSIDE = -4, /* |l_camera| > max_radius: panic at src/systems.rs:122-124 */
  CURVIS_E_NO_SKY = -5,         /* a background image has not been set */
  CURVIS_E_PARALLEL = -6,       /* forward/up parallel: panic at src/algebra.rs:19-21 */
  CURVIS_E_METRIC = -7,         /* invalid metric parameters: panics at src/metrics.rs:409-456 */
  CURVIS_E_RCCL = -8,           /* RCCL call failed */
  CURVIS_E_SAMPLING = -9,       /* sampler panic (< 3 finite points): src/sampling.rs:155-157 */
  CURVIS_E_IO = -10
};

/* enum Metric (src/metrics.rs:575-578) + FlatSphericalMetric (src/metrics.rs:492-505) */
enum { CURVIS_METRIC_ELLIS = 0, CURVIS_METRIC_INTERSTELLAR = 1, CURVIS_METRIC_FLAT = 2, CURVIS_METRIC_SCHWARZSCHILD = 3 };

/* CURVIS_METRIC_SCHWARZSCHILD: a Schwarzschild black hole of mass M (field `m`; `rho` and `a` are ignored; valid iff m > 0), a kind the
 * reference does not have.  It fits the reference's trait DiagonalSphericalMetric (g00 = -1, g11 = 1, one function r(l)) through the OPTICAL
 * metric: null geodesics and the angles a static observer measures are conformally invariant, and Schwarzschild's metric divided by
 * (1 - 2M/r), written in the tortoise coordinate, has exactly the trait's form,
 *     l    = r + 2M log(r/2M - 1)           r the areal radius, r > 2M
 *     R(l) = r / sqrt(1 - 2M/r)             what the trait calls r(l)
 * R has its minimum 3 sqrt(3) M at the photon sphere (r = 3M, l = 1.614 M), R -> |l| for l -> +inf, and R grows without bound for
 * l -> -inf, the horizon.  In this picture the hole is a wormhole whose far side is the horizon: a ray is captured exactly when it
 * escapes to -l, so the escape test, the which-side code and the counters (n_neg = captured rays) are the ones every kind has, and the
 * sky set for -l is "what is painted on the horizon" -- set an opaque black one and the shadow appears.  What is represented: the null
 * geodesics and the local angles of Schwarzschild, for a camera that is a static observer at areal radius r(l_camera).  What is not:
 * proper time and redshift (curvis_metric_functions and curvis_metric_tensor return the optical metric, whose g00 is -1) -- the
 * one exception is the emission of a moving accretion disc (curvis_ctx_set_disc_motion), which is scaled by the physical metric's
 * frequency ratio.
 *
 * Definition of R, R^2 and R' at l -- an explicit sequence of individually rounded FP64 operations, one text for host and device
 * (cv_device.h metric_eval, cv_math.h cv_tortoise_u), a pure function of l: no iteration count that depends on the data, nothing
 * carried over from the previous step.  inv = RN(1 / (2M)) and 2M (exact) are formed once per call on the host.
 *   0. lc = l < 0 ? 0 : l                                (the funnel, below; -0 and +0 give the same y; a NaN stays)
 *   1. y  = fma(lc, inv, -1)                             l/2M - 1; with u = r/2M - 1 > 0 the tortoise relation reads u + log u = y
 *   2. guess:  y < 2:  t = y - 1,  u = fma(t, fma(t, fma(t, -1/192, 1/16), 1/2), 1)       (Taylor polynomial of u(y) at y = 1)
 *              else:   L = log y,  u = (y - L) + L / y                                     (asymptotic series)
 *   3. four times:  u = u + (u * ((y - u) - log u)) / (1 + u)                              (Newton on u + log u - y, correction form)
 *   4. w = 1 + u,  q = sqrt(u * w)
 *   5. R  = ((2M * w) * w) / q                           = 2M (1 + u)^(3/2) / sqrt(u)
 *      R' = (2 * u - 1) / (2 * q)                        = dR/dl = (2u - 1) / (2 sqrt(u (1 + u)))
 *      R^2 = R * R
 * log is cv_math.h's cv_log_t (full domain); every quotient and the root are the correctly rounded ones (IEEE `/` and sqrt on the
 * host, their Markstein forms on the device -- never a bare hardware seed).  Measured against mpmath at 40 digits
 * (profiles/schwarzschild_accuracy.txt): R within 3.3 ulp; R' passes through zero at the photon sphere, where the error of u (about an ulp)
 * is up to 6 400 ulp of the small R'.  Bit-for-bit agreement of host and device is
 * asserted for 2^-90 <= M < 2^88 and |l| < 2^90 (the fast step's guard); outside, a quotient of the device may lose its last bit.
 *
 * The funnel.  For l < 0 (y < -1, u < 0.2785, r < 2.557 M: well inside the photon sphere) the three functions are DEFINED as their
 * values at l = 0: R is constant and R' < 0 is constant, so dp_l = b^2 R' / R^3 <= 0 and a ray that enters l < 0 moving inward keeps
 * p_l < 0 and reaches -max_radius.  No ray that escapes to +l ever goes below the photon sphere, so the region is never seen and the
 * solver never needs exp or arguments below y = -1.  The funnel is a capture device, not physics.  A render call whose camera has
 * l <= 0 fails with CURVIS_E_INVALID under this kind.
 *
 * Kernels: the static kernel (fused, with every option, and the debug dump's staged form), both step flavours, the samplers, the
 * direct renderer and trajectories.  There is no relay and no persistent kernel of the kind: the automatic choice and "variant" = 2 take
 * the static kernel, and "variant" = 0 is refused with CURVIS_E_INVALID. */

/* EllisMetric { rho } (src/metrics.rs:399-401), InterstellarMetric { m, a, rho } (:431-435). */
typedef struct curvis_metric {
  int32_t kind;
  int32_t _pad;
  double rho, m, a;
} curvis_metric;

/* Camera (src/cameras.rs:16-34) reduced to what the kernels read: position (t,l,theta,phi),
 * camera_to_world_rotation_matrix (row-major), focal_length, sensor_width/height, resolution. */
typedef struct curvis_camera {
  double pos[4];
  double rot[9];
  double focal, sensor_w, sensor_h;
  uint32_t res_x, res_y;
} curvis_camera;

/* PhotonEscape (src/systems.rs:39-44) */
enum { CURVIS_NOT_ESCAPED = 0, CURVIS_POSITIVE_SPACE = 1, CURVIS_NEGATIVE_SPACE = -1 };
/* not in the reference: the ray ended on the context's disc (below) */
enum { CURVIS_DISC = 2 };

/* per-ray final state, for parity tests: RelativisticObject (src/vectors.rs:135-139) after
 * escape_photon, number of Euler steps executed, escape code, raw texel indices
 * (`as u32` results of src/images.rs:118-119, before clamping). */
typedef struct curvis_ray_debug {
  double x[4];
  double p[4];
  uint32_t steps;
  int32_t code;
  uint32_t tx, ty;
} curvis_ray_debug;

typedef struct curvis_stats {
  uint64_t rays;      /* rays traced */
  uint64_t steps;     /* Euler steps executed (sum over rays) */
  uint64_t n_pos;     /* escaped to +l */
  uint64_t n_neg;     /* escaped to -l */
  uint64_t n_none;    /* hit the iteration cap */
  uint64_t n_oob;     /* texel index == W or == H (reference would panic); clamped */
  double kernel_ms;   /* HIP-event time of the kernels on the context's stream (integrate + shade) */
  double total_ms;    /* wall time of the call including H2D/D2H */
  double integrate_ms; /* HIP-event time of the geodesic integration kernel(s) alone */
  double shade_ms;     /* HIP-event time of the shading (direction + sky lookup) kernel(s) */
} curvis_stats;

typedef struct curvis_ctx curvis_ctx;

const char *curvis_version(void);
/* message of the last error on this context (or of the last failed curvis_ctx_create if ctx == NULL) */
const char *curvis_last_error(const curvis_ctx *ctx);
int curvis_device_count(void);

int curvis_ctx_create(int device, curvis_ctx **out);
void curvis_ctx_destroy(curvis_ctx *ctx);
/* name of the device + number of CUs, for bench reports */
int curvis_ctx_device_info(const curvis_ctx *ctx, char *name, size_t name_cap, int *compute_units, int *clock_mhz);
/* which physical GPU this context sits on and what it is doing right now, for the per-device tables of multi-GPU runs
 * (bench.py `per_rank`, `curvis video --stats`): PCI address "dddd:bb:dd.f" (hipDeviceGetPCIBusId), the current
 * shader clock in MHz and the board power in W as the amdgpu driver reports them in sysfs (pp_dpm_sclk,
 * hwmon power1_average / power1_input); a value that cannot be read comes back as -1, never as an error.  No
 * reference counterpart (the reference is single-threaded CPU code). */
int curvis_ctx_device_status(const curvis_ctx *ctx, char *pci_bus_id, size_t cap, int *sclk_mhz, int *power_w);

/* SphericalImage (src/images.rs:51-56): which = 0 -> background_positive (+l), 1 -> background_negative.
 * `rgba` is the decoded image as Rgba8 (what DynamicImage::get_pixel returns, src/images.rs:107-111),
 * row-major, host memory; it is copied to HBM and kept for all frames. */
int curvis_ctx_set_sky(curvis_ctx *ctx, int which, const uint8_t *rgba, uint32_t w, uint32_t h);
/* same, from a device pointer on this context's GPU (e.g. a buffer filled by an RCCL broadcast);
 * copy != 0 copies it, copy == 0 borrows it (caller keeps it alive).  With option "sky_mipmap" a borrowed buffer is level 0 of the
 * mip chain, whose other levels are built from it once: a caller who rewrites the buffer calls this function again. */
int curvis_ctx_set_sky_device(curvis_ctx *ctx, int which, const void *dev_rgba, uint32_t w, uint32_t h, int copy);
/* SphericalImage::set_forward_up (src/images.rs:102-104); default forward = x, up = z. */
int curvis_ctx_set_sky_orientation(curvis_ctx *ctx, int which, const double forward[3], const double up[3]);
/* Broadcast both sky textures from rank `root` over an existing RCCL communicator (ncclComm_t):
 * the shapes (4 x u32) first, then two ncclBroadcast calls of w*h*4 bytes each over xGMI.
 * Non-root ranks need no prior set_sky: their textures are allocated from the broadcast shapes. */
int curvis_ctx_bcast_skies(curvis_ctx *ctx, void *nccl_comm, int root);

/* RCCL plumbing for a host that has no RCCL binding of its own (one process per GPU -- a Rust host, `bench.py`):
 * rank 0 draws an id (ncclGetUniqueId) and ships its CURVIS_RCCL_ID_BYTES bytes to the other processes by whatever
 * out-of-band channel it has; every process then joins with its own context (ncclCommInitRank on the context's
 * device) and passes the returned communicator to curvis_ctx_bcast_skies.  The communicator is the caller's:
 * curvis_rccl_comm_destroy it after the broadcast.  A one-process / N-thread host (`curvis video --devices N`) needs
 * none of this: it calls ncclCommInitAll itself.  Single node by design (frames shard over the GPUs of ONE node): unless
 * NCCL_SOCKET_IFNAME is set these two calls set it to "lo", so RCCL's bootstrap does not wait on an unroutable interface.
 * No reference counterpart (single-threaded CPU code). */
#define CURVIS_RCCL_ID_BYTES 128
int curvis_rccl_unique_id(uint8_t id[CURVIS_RCCL_ID_BYTES]);
int curvis_ctx_rccl_comm_init(curvis_ctx *ctx, const uint8_t id[CURVIS_RCCL_ID_BYTES], int n_ranks, int rank,
                              void **comm_out);
int curvis_rccl_comm_destroy(void *nccl_comm);

/* Read back `bytes` bytes at byte offset `offset` of sky texture `which` from HBM (e.g. to verify on every rank that
 * a broadcast texture equals the root's file). */
int curvis_ctx_read_sky(curvis_ctx *ctx, int which, size_t offset, size_t bytes, uint8_t *out);
/* Level `level` of the mip chain of sky `which` (option "sky_mipmap" below; level 0 is the sky), built on the context's stream if it
 * is not there yet: *w x *h RGBA8 texels into `out` (NULL: the size alone).  CURVIS_E_NO_SKY without a sky, CURVIS_E_INVALID for a
 * level the chain does not have.  For tests and tools. */
int curvis_ctx_sky_mip_level(curvis_ctx *ctx, int which, uint32_t level, uint8_t *out, uint32_t *w, uint32_t *h);

/* The accretion disc (not in the reference): one object at finite distance, a thin textured annulus in the equatorial plane, seen by
 * the brute renderer.  A context may hold one disc: an RGBA8 texture D of w x h texels, w along azimuth and h along l, and two finite
 * doubles l_inner < l_outer of either sign.  The bounds are in the radial coordinate l, not in r(l): l is monotonic in every metric
 * kind (the Schwarzschild kind's R(l) is not), and negative values put the disc on the far side of a wormhole.  The disc lies in the
 * plane theta = pi/2 (mod pi), is infinitely thin, opaque where its texel's alpha is >= 128 and absent where it is < 128, and emits its
 * texel's colour: no redshift, no Doppler shift, no beaming (see what the Schwarzschild paragraph says is not represented) -- unless
 * the disc is given a motion, curvis_ctx_set_disc_motion below.
 *
 * Notation for a ray.  y_0 is the photon at the camera, y_k the state after k steps of whatever the call's step is (the Euler step,
 * "step_scale"'s step, or a Heun step; the stage states of a Heun step are not states).  (s_k, c_k) is the one cv_math.h sincos
 * evaluation of theta_k that the step from y_k performs anyway (under Heun: its first stage's).  It is defined only for states a step
 * is taken from -- not escaped, and k < max_iterations: the final state of an escaping or capped ray is never tested.  The cosine of
 * a double is never zero.
 * For k >= 1, before the step from y_k is counted:
 *   1. The ray crossed the plane iff (c_{k-1} < 0) != (c_k < 0).
 *   2. t = c_{k-1} / (c_{k-1} - c_k), the correctly rounded quotient (IEEE `/` on the host, a Markstein form on the device -- never a
 *      bare hardware seed).
 *   3. l_hit = l_{k-1} + t (l_k - l_{k-1}) and phi_hit = phi_{k-1} + t (phi_k - phi_{k-1}), each operation individually rounded, in
 *      that order, no fma.
 *   4. The crossing is on the disc iff l_inner <= l_hit && l_hit <= l_outer (a NaN fails both compares).
 *   5. If s_k < 0: phi_hit = phi_hit + pi.  A ray whose theta has left [0, pi] is physically at azimuth phi + pi -- what the sky
 *      lookup's normalize_theta_phi does, with the same constant pi.
 *   6. Column: tx = min(as_u32((rem_euclid(phi_hit, 2 pi) / (2 pi)) * (double)w), w - 1), with the sky lookup's rem_euclid and `as u32`
 *      and a correctly rounded quotient.
 *   7. Row: ty = min(as_u32(((l_hit - l_inner) / (l_outer - l_inner)) * (double)h), h - 1).
 *   8. If alpha(D[ty][tx]) >= 128 the ray ends here: its code is CURVIS_DISC, its step count is k, its colour is the RGB of D[ty][tx].
 *      It counts in rays and steps and in the per-frame counter n_disc (curvis_ctx_frame_disc_hits), and in none of n_pos, n_neg,
 *      n_none, n_oob: per frame, rays = n_pos + n_neg + n_none + n_disc.
 *   9. Otherwise the ray goes on as if nothing had been there.
 * The colour goes where a sky colour goes: under "supersample" sub-rays on the disc are averaged with sub-rays on the sky;
 * "sky_filter" does not filter it; under "sky_mipmap" a disc ray is a quad partner that saw no sky.  Steps 1-7 are one function for
 * host and device (cv_device.h disc_crossing); curvis_disc_crossing is its host accessor.
 *
 * curvis_ctx_set_disc copies the texture (host memory, w * h * 4 bytes, row-major) to the device; rgba == NULL removes the disc.
 * CURVIS_E_INVALID for w == 0, h == 0, a bound that is not finite, or !(l_inner < l_outer); the disc that was set before stays.  The
 * disc belongs to the context: curvis_ctx_bcast_skies does not carry it.  While a disc is set, curvis_render_brute, _rows and _batch
 * honour it, with every option, through the static kernel (never the relay kernel); refused with CURVIS_E_INVALID and a message that
 * names the disc are curvis_render_efficient, curvis_render_efficient_batch, curvis_ctx_prefetch_efficient and curvis_render_direct
 * (both renderers reduce every ray to an equatorial orbit that depends on one angle: there is no theta), curvis_render_brute_debug,
 * "variant" = 0 and "fuse_shade" = 0 (the staged paths have no slot for a disc colour).  curvis_photon_trajectories,
 * curvis_compute_escape_angles and curvis_walk_ray do not see it.  With no disc set every call launches exactly the kernels it
 * launched before there was one. */
int curvis_ctx_set_disc(curvis_ctx *ctx, const uint8_t *rgba, uint32_t w, uint32_t h, double l_inner, double l_outer);
/* The disc's emission shift (not in the reference): the disc gets a motion sigma in {0, +1, -1} and a gain G.  sigma = 0 is the disc of
 * the paragraph above, bit for bit, and G is not applied.  With sigma = +-1 the disc's matter moves on circular geodesics of
 * Schwarzschild in the +-phi direction, Omega = sigma sqrt(M / r^3), and the camera is the static observer the project assumes
 * everywhere.  A ray is traced with covariant momentum p_t = 1 and constant p_phi (its angular momentum about the disc's axis: the disc
 * lies in the coordinate equator); covariant components are conformally invariant, so the optical-metric ray carries the p_t, p_phi of
 * the physical one.  The frequency ratio of a ray that ends on the disc at l_hit (r_e there, r_c at the camera; the sign of the
 * past-directed tracing cancels in the ratio) is
 *   g = sqrt(1 - 3M/r_e) / (sqrt(1 - 2M/r_c) (1 + Omega p_phi)),
 * and the emitted colour is scaled by the bolometric factor F = G g^4: Doppler shift, beaming and gravitational redshift in one
 * number, no change of hue.  In the kind's own variable u = r/2M - 1 that is one square root and no fourth root.  F is DEFINED as this
 * sequence, every operation individually rounded, no fma:
 *   1. u_e = schwarzschild_u(M, l_hit) and u_c = schwarzschild_u(M, l_camera): the kind's function (curvis_schwarzschild_u), its
 *      l < 0 funnel included.  l_camera is the frame's camera coordinate, l_hit the value of step 3 above.
 *   2. w = 1 + u_e and n = 2 u_e - 1.  If !(n > 0): F = 0 -- at or inside the photon sphere r = 3M, where there is no circular orbit;
 *      the ray still ends on the disc, and is painted black.
 *   3. a = n / (2 w).  This is 1 - 3M/r_e.
 *   4. om = RN(1/2M) / (w sqrt(2 w)).  This is |Omega|; RN(1/2M) is the constant the kind already carries.
 *   5. den = 1 + (sigma om) p_phi.  If !(den > 0): F = 0.  In exact arithmetic |Omega p_phi| < 1 outside r = 3M: the null condition
 *      of the optical metric, p_l^2 + (p_theta^2 + p_phi^2 / sin^2 theta) / R^2 = 1, gives |p_phi| <= R(r) in the equator, and
 *      Omega R = sqrt(M / r^3) r / sqrt(1 - 2M/r) = sqrt(M / (r - 2M)), which is below 1 exactly when r > 3M.  The test keeps a
 *      caller's oversized p_phi (curvis_disc_shift takes any) and the roundings next to r = 3M from a negative or infinite g.
 *   6. A_c = u_c / (1 + u_c).  This is 1 - 2M/r_c.
 *   7. g2 = a / (A_c (den den)).
 *   8. F = G (g2 g2).
 * The quotients are the correctly rounded ones, the root is IEEE's.  Colour: for each of the three 8-bit channels c of the texel,
 * v = (double)c F + 0.5 and c' = (v >= 255.0) ? 255 : as_u32(v) (`as u32`: truncation, NaN and negatives to 0; a NaN cannot occur after
 * steps 2 and 5 for a ray the renderer traced).  Alpha is kept, so "non-zero texel = ended on the disc" still holds.  The shifted colour
 * replaces the texel's colour everywhere the paragraph above speaks of it: in the "supersample" average, in the "sky_filter" and
 * "sky_mipmap" branches that take the disc ray's own colour, in row bands and in batches (each frame with its own camera's u_c).
 * Codes, step counts and every counter, n_disc included, are those of sigma = 0.  Steps 1-8 are one function for host and device
 * (cv_device.h disc_shift, the colour disc_shade); curvis_disc_shift and curvis_disc_shade are the host accessors.
 *
 * curvis_ctx_set_disc_motion: motion = sigma, gain = G; the default is (0, 1.0).  CURVIS_E_INVALID for a motion outside {-1, 0, 1} or a
 * gain that is not finite or is negative; the former values then stay.  The setting belongs to the context, survives
 * curvis_ctx_set_disc (also the removal of the disc) and does nothing without a disc.  A brute render call (curvis_render_brute, _rows,
 * _batch) with a disc, motion != 0 and a metric kind other than CURVIS_METRIC_SCHWARZSCHILD is refused with CURVIS_E_INVALID and a
 * message that names the disc motion: the wormhole kinds and flat space have g_00 = -1, free matter there is at rest, and nothing is
 * Keplerian.  Every refusal of the paragraph above stays.  With motion = 0 every call launches exactly the kernels it launched before
 * there was a motion. */
int curvis_ctx_set_disc_motion(curvis_ctx *ctx, int motion, double gain);
/* Steps 1-8 above on the host (no GPU needed): *F for a Schwarzschild metric `m`, the crossing's l_hit, the camera's l, motion (+-1;
 * 0 gives *F = gain's neutral value 1.0: the colour is the texel's), gain and the ray's p_phi, all taken as they are.
 * CURVIS_E_INVALID for a null pointer, a metric that is not of kind CURVIS_METRIC_SCHWARZSCHILD, or a motion outside {-1, 0, 1};
 * CURVIS_E_METRIC for a metric curvis_metric_validate refuses. */
int curvis_disc_shift(const curvis_metric *m, double l_hit, double l_camera, int motion, double gain, double p_phi, double *F);
/* The colour rule above for one RGBA8 texel (red in the low byte): *out = the texel with its three colour channels scaled by F, alpha
 * kept.  CURVIS_E_INVALID for a null pointer. */
int curvis_disc_shade(uint32_t texel, double F, uint32_t *out);
/* Steps 1-7 of the disc's paragraph for one pair of consecutive states, on the host (no GPU needed): *hit = 1 when the ray crossed the plane inside
 * [l_inner, l_outer], and then (*tx, *ty) is the texel; *hit = 0 otherwise (tx, ty = 0).  The alpha test of step 8 is the caller's.
 * CURVIS_E_INVALID for a null pointer, w == 0 or h == 0; the bounds are taken as they are. */
int curvis_disc_crossing(double c_prev, double c_cur, double s_cur, double l_prev, double l_cur, double phi_prev, double phi_cur,
                         double l_inner, double l_outer, uint32_t w, uint32_t h, int32_t *hit, uint32_t *tx, uint32_t *ty);

/* how two devices of this node are connected (hipExtGetLinkTypeAndHopCount, hipDeviceCanAccessPeer, hipDeviceGetP2PAttribute):
 * link_type = HSA_AMD_LINK_INFO_TYPE_* (2 PCIe, 4 xGMI; 0 with hops 0 for a == b; -1 unknown).  Read beside the measured
 * sky-broadcast rate: xGMI is point-to-point, 7 links x ~153 GB/s per MI355X.  Output pointers may be NULL.  The errors of
 * curvis_ctx_bcast_skies / curvis_ctx_rccl_comm_init name the stage that failed ("sky broadcast, stage header_broadcast: ...")
 * and carry RCCL's own last error. */
int curvis_device_link(int device_a, int device_b, int *link_type, int *hops, int *peer_access, int *performance_rank,
                       int *native_atomics);

/* Camera::new (src/cameras.rs:79-122) incl. Orientation::new (src/algebra.rs:16-38). */
int curvis_camera_init(curvis_camera *out, const double pos[4], const double forward[3], const double up[3],
                       double focal_length, double sensor_diagonal, uint32_t res_x, uint32_t res_y);
/* Orientation::new: rotation matrix, its inverse and the orthogonalised up (any may be NULL). */
int curvis_orientation_init(const double forward[3], const double up[3], double rot[9], double inv_rot[9],
                            double up_out[3]);
/* EllisMetric::new / InterstellarMetric::new parameter checks (src/metrics.rs:407-459); Schwarzschild: m > 0 (false for a NaN). */
int curvis_metric_validate(const curvis_metric *m);
/* The three required methods of trait DiagonalSphericalMetric (src/metrics.rs:40-48: r, r_squared, r_derivative;
 * Ellis :417-421, Interstellar :467-485, flat :501-505) at radial coordinate l, evaluated on the host with the same
 * arithmetic (cv_math.h) the kernels use -- what every ray of a render is integrated with.  Any output may be NULL. */
int curvis_metric_functions(const curvis_metric *m, double l, double *r, double *r_squared, double *r_derivative);
/* CURVIS_METRIC_SCHWARZSCHILD only (any other kind: CURVIS_E_INVALID): u = r/2M - 1 at radial coordinate l as steps 0-3 of the kind's
 * definition above compute it -- the number R and R' are formed from (R' has the sign of 2u - 1 exactly). */
int curvis_schwarzschild_u(const curvis_metric *m, double l, double *u);
/* The diagonal of the metric tensor at `position` = (t, l, theta, phi): covariant g_ii = (-1, 1, r^2(l),
 * r^2(l) sin^2(theta)) (src/metrics.rs:49-68; sin().powi(2) is s * s) and contravariant g^ii = g_ii.powi(-1) = 1 / g_ii
 * (:84-93) -- what to_covariant / to_contravariant (:163-219) multiply a vector's components by.  Host-side, same
 * arithmetic as the kernels; either output may be NULL. */
int curvis_metric_tensor(const curvis_metric *m, const double position[4], double g_cov[4], double g_contr[4]);

/* RelativisticSystem::render_image (src/systems.rs:307-330): one ray per pixel, forward-Euler
 * integration until |l| > max_radius or max_iterations steps, nearest-texel sky lookup.
 * rgb_out: host buffer res_y*res_x*3 (row-major, RGB8) or NULL to leave the frame in HBM
 * (see curvis_ctx_framebuffer / curvis_ctx_download). */
int curvis_render_brute(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                        uint32_t max_iterations, double max_radius, double delta, uint8_t *rgb_out,
                        curvis_stats *stats);
/* Host-side accessors of the per-ray functions either end of the Euler loop, in the kernels' arithmetic (the same
 * host/device source): what the kernels do for every pixel, callable for one.
 * Camera::outward_vector_on_camera_space (src/cameras.rs:150-164; unit vector, x forward / y left / z up) and
 * outward_vector_on_world_space_from_x_y (:169-172, the former rotated by camera_to_world); either output may be NULL. */
int curvis_camera_outward_vector(const curvis_camera *camera, uint32_t px, uint32_t py, double camera_space[3],
                                 double world_space[3]);
/* The same for option "projection" (defined with the options below): the unit camera-space vector of pixel (px, py) under
 * projection 0, 1 or 2 -- the un-normalised vec of the definition through the reference's normalize -- and its rotation into world
 * space.  Projection 0 is curvis_camera_outward_vector bit for bit; any other value than 0, 1, 2 is CURVIS_E_INVALID.  The fisheye
 * range check is made by the render calls, not here. */
int curvis_camera_outward_vector_projected(const curvis_camera *camera, int32_t projection, uint32_t px, uint32_t py,
                                           double camera_space[3], double world_space[3]);
/* The moving camera (not in the reference, whose cameras are static observers): relativistic aberration.  A frame may be given the
 * velocity beta = (b_l, b_theta, b_phi) of its camera: the components, in units of c, that the static observer at the camera's position
 * measures, in the tangent frame `forward` and `up` live in (camera.rot maps camera space into it).  For the Schwarzschild kind, whose
 * rays are those of the optical metric, beta is the optical-metric speed with respect to coordinate time; conformal invariance keeps
 * everything below unchanged.  A pixel then looks along the direction the static observer assigns to what the moving camera sees along
 * that pixel.  Every operation is one individually rounded FP64 operation in the order written, without contraction; square roots and
 * quotients are the correctly rounded IEEE ones.
 * Once per frame (curvis_camera_boost_prepare; rot[r][i] = camera.rot[3 r + i]):
 *   1. c_i = ((rot[0][i] b_l) + rot[1][i] b_theta) + rot[2][i] b_phi for i = 0, 1, 2: the camera-space velocity.
 *   2. b2 = (c_0 c_0 + c_1 c_1) + c_2 c_2.
 *   3. b2 == 0: the frame is not boosted; its pixels are those of a call without a velocity, bit for bit.
 *   4. !(b2 < 1.0), a NaN included: CURVIS_E_INVALID.
 *   5. b = sqrt(b2), g = 1.0 / sqrt(1.0 - b2), u_i = c_i / b, A = g - 1.0, B = g b.
 * Per ray, with vec = (x, y, z) the un-normalised camera-space vector of the pixel under the call's "projection":
 *   1. n = sqrt((x x + y y) + z z).
 *   2. p = (x u_0 + y u_1) + z u_2.
 *   3. s = A p - B n.
 *   4. vec' = (x + u_0 s, y + u_1 s, z + u_2 s).
 * The reference's sequence (normalize, the rotation, new_photon) continues with vec'.  Up to that normalisation vec' is
 * (gamma (d_par - beta), d_perp) for a pixel that looks along d in the camera's rest frame: cos theta_static = (cos theta' - beta) /
 * (1 - beta cos theta').  Both functions are one text for host and device (cv_device.h camera_boost_prepare, camera_boost).
 * This is aberration and nothing else: no Doppler shift and no beaming of the sky, no light-travel-time effect, no acceleration, and
 * the camera's motion does not enter the emission shift of a moving disc.
 *
 * curvis_ctx_set_camera_velocities: beta holds 3 n doubles, one triple per frame; n = 0 or beta = NULL clears them.  The state belongs
 * to the context and stays until it is set again.  CURVIS_E_INVALID (the former state stays) for a triple whose own
 * (b_l b_l + b_theta b_theta) + b_phi b_phi is not below 1.  A render call of F frames -- every renderer: curvis_render_brute, _rows,
 * _batch, curvis_render_efficient, _batch, curvis_render_direct -- takes triple f for its frame f when n == F, the one triple for every
 * frame when n == 1, and is refused with CURVIS_E_INVALID, rendering nothing, for any other n != 0.  Steps 1-5 run at call time with
 * each frame's own rot.  It works with every metric kind and every option, and with a disc whose motion is 0.  While a frame of the
 * call moves, curvis_render_brute_debug, "variant" = 0, "fuse_shade" = 0 and a disc with a motion other than 0 are refused under the
 * name "camera velocity", and the brute renderer takes the static kernel.  With the velocities cleared, or all of them zero, every
 * call launches the kernels it launched before. */
int curvis_ctx_set_camera_velocities(curvis_ctx *ctx, const double *beta, uint32_t n);
/* Steps 1-5 above on the host (no GPU needed): out = (u_0, u_1, u_2, A, B), all zeros for a frame that is not boosted (a boosted one has
 * B > 0).  CURVIS_E_INVALID for a null pointer or step 4. */
int curvis_camera_boost_prepare(const curvis_camera *camera, const double beta[3], double out[5]);
/* curvis_camera_outward_vector_projected for a camera with velocity beta: vec' through the reference's normalize, and its rotation into
 * world space; either output may be NULL.  beta = 0 gives that function's bits. */
int curvis_camera_outward_vector_boosted(const curvis_camera *camera, int32_t projection, const double beta[3], uint32_t px, uint32_t py,
                                         double camera_space[3], double world_space[3]);
/* The velocity of a camera on a path, from three consecutive poses pos = (t, l, theta, phi) (the first frame passes pos_prev = pos, the
 * last pos_next = pos: a one-sided difference) and the speed of light in path units per unit of t:
 *   dt = t_next - t_prev, inv = 1.0 / (dt light_speed),
 *   b_l = (l_next - l_prev) inv, b_theta = r(l) (theta_next - theta_prev) inv, b_phi = (r(l) sin theta) (phi_next - phi_prev) inv
 * with the kind's r(l) and cv_math.h's sine at the middle pose, every product and difference rounded once, left to right; dt == 0 gives
 * zero.  The angle differences are taken as they are: a path whose phi jumps by 2 pi between frames must be unwrapped by the caller.
 * Nothing is checked against the speed of light here. */
int curvis_camera_path_velocity(const curvis_metric *metric, const double pos_prev[4], const double pos[4], const double pos_next[4],
                                double light_speed, double beta_out[3]);
/* DiagonalSphericalMetric::relativistic_vector_to_direction (src/metrics.rs:339-349 with to_contravariant :190-203):
 * covariant momentum at `position` -> tangent-space direction (not normalised; z uses frame_field_22, as the
 * reference does). */
int curvis_vector_to_direction(const curvis_metric *metric, const double position[4], const double p_cov[4],
                               double direction[3]);
/* DiagonalSphericalMetric::update_relativistic_object (src/metrics.rs:283-297) for a covariant momentum: ONE forward-Euler
 * step of (x, p_cov) in place, on the host, with the IEEE form of the step the kernels fall back to (the fast step
 * returns the same bits) -- the body of curvis_photon_trajectories' loop, all eight components. */
int curvis_update_relativistic_object(const curvis_metric *metric, double x[4], double p_cov[4], double delta);
/* Option "step_scale" (defined with the options below) for ONE step: *out = delta_k, the step a render call with step `delta` under
 * step_scale = S takes from a ray whose radial coordinate before the step is l -- kappa formed as the render calls form it, then
 * cv_device.h step_delta, the text the kernels' loops call.  S = 0 gives delta.  CURVIS_E_INVALID for S outside [0, 2^20], a null
 * `out`, and S != 0 with !(delta > 0).  Fed into curvis_update_relativistic_object it walks a ray the way the kernels do. */
#define CURVIS_STEP_SCALE_MAX (1u << 20)
int curvis_step_delta(double delta, int64_t step_scale, double l, double *out);
/* A whole ray on the host: from (x, p_cov), in place, the loop the render kernels run -- step size from curvis_step_delta's text (S = step_scale),
 * one step of curvis_update_relativistic_object (integrator = 0) or curvis_heun_step (1), the escape test |l| > max_radius, at most
 * max_iterations steps -- with the IEEE form of the step.  *steps and *code (CURVIS_POSITIVE_SPACE, CURVIS_NEGATIVE_SPACE, CURVIS_NOT_ESCAPED)
 * are what curvis_render_brute_debug records for the ray; x[0] is its time.  One call instead of one per step for host-side references.
 * CURVIS_E_INVALID for a null pointer, an integrator other than 0 or 1, S outside [0, 2^20], and S != 0 or integrator = 1 with !(delta > 0). */
int curvis_walk_ray(const curvis_metric *metric, double x[4], double p_cov[4], double delta, int64_t step_scale, int32_t integrator,
                    uint32_t max_iterations, double max_radius, uint32_t *steps, int32_t *code);
/* Option "integrator" = 1 (defined with the options below) for ONE step: a Heun step of (x, p_cov) in place, on the host, all eight
 * components, with the IEEE form of the Euler step (cv_device.h ray_step_heun, the text the kernels' loops call; the fast step
 * returns the same bits).  x[0] is averaged like the other coordinates; p_cov[0] and p_cov[3] keep their bits.  With `delta` taken
 * from curvis_step_delta at x[1] it walks a ray the way the kernels do under both options.  Returns as
 * curvis_update_relativistic_object does. */
int curvis_heun_step(const curvis_metric *metric, double x[4], double p_cov[4], double delta);
/* SphericalImage::get_pixel_from_vector3's texel (src/images.rs:115-142, 171-174; src/algebra.rs:106-134) for an image of
 * w x h texels whose inverse orientation is inv_rot (NULL = the default forward x / up z): raw `as u32` indices.
 * Returns CURVIS_OK, or CURVIS_E_INVALID with the indices still set when x == w or y == h (the reference's
 * get_pixel panics there; the kernels clamp and count such rays, curvis_stats.n_oob). */
int curvis_sky_texel_index(uint32_t w, uint32_t h, const double inv_rot[9], const double v[3], uint32_t *x, uint32_t *y);
/* its sibling for option "sky_filter" = 1 (host only): steps 1-4 of the option's definition below for the direction v --
 * taps = {x0, x1, y0, y1, fx, fy}, raw = {X >> 8, Y >> 8} (what curvis_sky_texel_index returns for the same arguments).
 * Returns CURVIS_OK, or CURVIS_E_INVALID with the outputs still set when the ray is out of bounds (raw[0] >= w or raw[1] >= h),
 * and CURVIS_E_INVALID for w or h beyond 2^23 (raw set, taps zero: 256 w is no u32 any more). */
int curvis_sky_bilinear_taps(uint32_t w, uint32_t h, const double inv_rot[9], const double v[3], uint32_t taps[6] /* x0 x1 y0 y1 fx fy */,
                             uint32_t raw[2] /* X>>8, Y>>8 */);
/* The integer parts of option "sky_mipmap" on the host (the option's paragraph below has the definition; the kernels compile the same
 * text).  curvis_sky_mip_rho: the footprint of a ray at own = {Xc, Yc} on a sky w texels wide from its horizontal and vertical quad
 * partners' {Xc', Yc'}; a partner with ok = 0 contributes nothing.  curvis_sky_mip_level: level k and fraction f for a pyramid of
 * `levels` levels.  curvis_sky_mip_taps: steps 3-4 of the bilinear definition on level `level` of a w x h sky for (xc >> level,
 * yc >> level) -- taps = {x0, x1, y0, y1, fx, fy}, size = {w_level, h_level}.  curvis_sky_mip_mix: the blend of two packed RGBA8 level
 * colours.  curvis_sky_mip_pyramid: level `level` of the pyramid of a host image (out may be NULL: the size alone).  All return
 * CURVIS_OK, or CURVIS_E_INVALID for a null pointer, an empty or too large sky, a level the pyramid does not have, f > 255 or an index
 * outside the virtual sky. */
int curvis_sky_mip_rho(uint32_t w, const uint32_t own[2], const uint32_t horizontal[2], int32_t horizontal_ok, const uint32_t vertical[2],
                       int32_t vertical_ok, uint32_t *rho);
int curvis_sky_mip_level(uint32_t rho, uint32_t levels, uint32_t *k, uint32_t *f);
int curvis_sky_mip_taps(uint32_t w, uint32_t h, uint32_t level, uint32_t xc, uint32_t yc, uint32_t taps[6], uint32_t size[2]);
int curvis_sky_mip_mix(uint32_t ck, uint32_t ck1, uint32_t f, uint32_t *out);
int curvis_sky_mip_pyramid(const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t level, uint8_t *out, uint32_t *wl, uint32_t *hl);

/* A band of image rows [row_begin, row_begin + row_count) of the same frame: rays are independent
 * (src/systems.rs:316-326), so a single image can be split across GPUs by rows and assembled on the host
 * (SURVEY 8e).  rgb_out: row_count*res_x*3 or NULL; stats cover the band. */
int curvis_render_brute_rows(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                             uint32_t row_begin, uint32_t row_count, uint32_t max_iterations, double max_radius,
                             double delta, uint8_t *rgb_out, curvis_stats *stats);
/* same as curvis_render_brute, plus the final state of every ray (dbg_out: res_y*res_x entries, row-major). */
int curvis_render_brute_debug(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                              uint32_t max_iterations, double max_radius, double delta, uint8_t *rgb_out,
                              curvis_ray_debug *dbg_out, curvis_stats *stats);
/* n_frames cameras of identical resolution rendered by ONE launch (video shards):
 * rgb_out is n_frames*res_y*res_x*3 or NULL. */
int curvis_render_brute_batch(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras,
                              uint32_t n_frames, uint32_t max_iterations, double max_radius, double delta,
                              uint8_t *rgb_out, curvis_stats *stats);

/* RelativisticSystem::render_image_efficient (src/systems.rs:333-527) -- what `curvis image` and
 * `curvis video` call (src/rendering.rs:97-106, :299-307): adaptive 1-D sampling of the escape angle over
 * alpha in [-0.1 pi, 1.1 pi] on the equatorial plane (src/sampling.rs), linear interpolation per pixel
 * (interp 1.0.3), axis-angle rotation of the camera direction, nearest-texel lookup.  Argument names and
 * order are the reference's.  Reproduces the reference's behaviour including the shrinking sample domain
 * (src/sampling.rs:161), extrapolation beyond the last sample and black +/- transitions.
 * CURVIS_E_SAMPLING where the reference panics: alpha_nums == 0 (`alpha_nums - 1` underflows, src/sampling.rs:133), and a
 * refinement round (max_iterations_sampling > 0) that starts with fewer than 3 finite samples (src/sampling.rs:155-157).
 * alpha_nums 1 and 2 are accepted: with max_iterations_sampling == 0 the frame is interpolated from a table of 0, 1 or 2
 * samples, as the reference's is (alpha_nums 1: the one grid point is 0 * inf = NaN, the table empty, every pixel black). */
int curvis_render_efficient(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                            uint32_t max_iterations_propagation, double max_radius, double delta, uint32_t alpha_nums,
                            uint32_t max_iterations_sampling, double sampling_convergence_threshold_1,
                            double sampling_convergence_threshold_2, uint8_t *rgb_out, curvis_stats *stats);
/* n_frames cameras: the per-frame samplers advance in lock step, one kernel launch per refinement round
 * for the whole batch, one per-pixel launch for all frames. */
int curvis_render_efficient_batch(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras,
                                  uint32_t n_frames, uint32_t max_iterations_propagation, double max_radius,
                                  double delta, uint32_t alpha_nums, uint32_t max_iterations_sampling,
                                  double sampling_convergence_threshold_1, double sampling_convergence_threshold_2,
                                  uint8_t *rgb_out, curvis_stats *stats);
/* The sampler of a FUTURE curvis_render_efficient_batch call, launched NOW on a stream of its own (device-resident sampler:
 * option "device_sampler").  Returns at once.  The render call with the same metric, settings and camera radii (the l of every
 * frame, in order) then finds its sample tables ready -- it waits for the sampler's event on its own stream instead of sampling --
 * so that a caller rendering batch after batch hides the sampler's latency (a handful of ~2000-step Euler chains on a few
 * compute units) under the previous batch's per-pixel kernel, PNG front end and host work:
 *     prefetch(batch 0); for k: { prefetch(batch k + 1); render(batch k); deflate / download(batch k); }
 * A prefetch nobody consumes costs its kernel and is overwritten by the second prefetch after it (two slots).  Settings the
 * device sampler does not take (alpha_nums beyond its arrays, a camera beyond max_radius) make this a no-op: the render call
 * deals with them.  Identical results with and without; read-only options "prefetches", "prefetch_hits",
 * "last_sampling_prefetched".  Reference seam: none -- the reference samples inside render_image_efficient
 * (src/systems.rs:437-486); this only moves WHEN the same sampling runs. */
int curvis_ctx_prefetch_efficient(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras, uint32_t n_frames,
                                  uint32_t max_iterations_propagation, double max_radius, double delta, uint32_t alpha_nums,
                                  uint32_t max_iterations_sampling, double sampling_convergence_threshold_1,
                                  double sampling_convergence_threshold_2);

/* "direct" mode -- NOT a function of the reference (SURVEY.md 8f N1 names it as an option): the image that
 * render_image_efficient approximates by adaptive sampling + linear interpolation, computed without either:
 * compute_escape_angle (src/systems.rs:203-261) is evaluated for the alpha of EVERY pixel (:405-433) and step 5
 * (:498-523) applied to its result.  A not-escaped photon, or one whose tangent rotation is undefined, gives a black
 * pixel (counted in n_none).  Parity: bit-exact against this repository's oracle (cvo_render_image_direct); against the
 * reference only through what it approximates (its efficient image differs where the interpolation does). */
int curvis_render_direct(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera, uint32_t max_iterations,
                         double max_radius, double delta, uint8_t *rgb_out, curvis_stats *stats);
/* sampler bookkeeping of the last efficient render (per frame): final table size, refinement rounds,
 * integrator calls, Euler steps, and whether the "maximum number of iterations" warning fired. */
typedef struct curvis_sampling_info {
  uint32_t n_samples, rounds;
  uint64_t calls, steps;
  int32_t warned_max_iterations;
  int32_t _pad;
} curvis_sampling_info;
int curvis_ctx_sampling_info(const curvis_ctx *ctx, uint32_t frame, curvis_sampling_info *info);
/* Statistics of frame `frame` of the last render call (brute, rows, batch, efficient, efficient batch): the
 * per-frame loop of VideoRenderingSystem::render (src/rendering.rs:291-316) is ONE launch per batch here, so the
 * kernels keep one set of counters per frame.  rays / steps / n_pos / n_neg / n_none / n_oob are exact for that
 * frame (for the efficient renderer: rays = pixels, steps = Euler steps of the frame's sampler, n_* = pixels by
 * escape space); the *_ms fields are the frame's share of the launch time (by executed steps), not a separate
 * measurement.  "last_frames" (curvis_ctx_get_option) = number of frames available. */
int curvis_ctx_frame_stats(const curvis_ctx *ctx, uint32_t frame, curvis_stats *stats);
/* n_disc of frame `frame` of the last render call, like curvis_ctx_frame_stats: the rays that ended on the disc (0 for a render
 * without a disc, and for the efficient and the direct renderer). */
int curvis_ctx_frame_disc_hits(const curvis_ctx *ctx, uint32_t frame, uint64_t *n_disc);
/* the (alpha, escape angle, escape space) table of a frame of the last efficient render; cap >= n_samples */
int curvis_ctx_samples(const curvis_ctx *ctx, uint32_t frame, double *alpha, double *escape_angle,
                       double *escape_space, size_t cap);

/* compute_escape_angles_range / compute_escape_angle (src/systems.rs:203-281, re-exported by src/lib.rs:37):
 * photons at (0, l, pi/2, 0) with tangent direction (cos a, 0, sin a); angle[i] = escape angle in [0, 2 pi)
 * (NaN when not escaped), space[i] = +1 / -1 / 0 (EscapeAngle::{PositiveSpace, NegativeSpace, NotEscaped}). */
int curvis_compute_escape_angles(curvis_ctx *ctx, const curvis_metric *metric, double l, const double *alphas,
                                 uint32_t n, double delta, uint32_t max_iterations, double max_radius,
                                 double *angle, int32_t *space, uint32_t *steps /* nullable */);
/* DiagonalSphericalMetric::new_photon (src/metrics.rs:301-334), host-side: position (t,l,theta,phi) and a
 * tangent-space direction -> contravariant position x and covariant momentum p. */
int curvis_new_photon(const curvis_metric *metric, const double position[4], const double direction[3], double x[4],
                      double p_cov[4]);
/* compute_photon_trajectory (src/systems.rs:77-92, re-exported by src/lib.rs:37) for n photons:
 * out[photon][iteration][0..7] = (x_t, x_l, x_theta, x_phi, p_t, p_l, p_theta, p_phi) BEFORE that iteration's
 * Euler step; momentum covariant. */
int curvis_photon_trajectories(curvis_ctx *ctx, const curvis_metric *metric, uint32_t n_photons, const double *x0,
                               const double *p0_cov, uint32_t iterations, double delta, double *out);

/* images::load_image / save_image (src/images.rs:7-20; image::open / DynamicImage::save of image 0.25.2) for the
 * two file formats this library decodes itself: PNG (every colour type and bit depth, converted to Rgba8 the way
 * DynamicImage::get_pixel does: grey -> (v, v, v, 255), 16 bit -> (v + 128) / 257, palette and tRNS expanded) and
 * JPEG (8-bit Huffman baseline / progressive; see csrc/host/jpeg_io.h on why JPEG is outside the pixel-parity
 * claims); the format is taken from the file's signature.  *rgba_out is w*h*4 bytes owned by the library until
 * curvis_image_free.  Errors: CURVIS_E_IO, message through curvis_last_error(NULL).  Host-only, no GPU needed. */
int curvis_image_load(const char *path, uint8_t **rgba_out, uint32_t *w, uint32_t *h);
void curvis_image_free(uint8_t *rgba);
/* DynamicImage::ImageRgb8(..).save(path) as PNG (8-bit RGB, non-interlaced) */
int curvis_image_save_rgb8(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h);
/* same with the encoder chosen: level -1 = the library's fast PNG writer (filter Up + one dynamic-Huffman block whose
 * only matches are zero runs: what `curvis video` writes its frames with; the reference's image crate also saves
 * with its fast setting), 0..9 = zlib at that level.  Same decoded pixels whatever the level. */
int curvis_image_save_rgb8_level(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h, int level);

/* PNG front end ON THE DEVICE, for hosts that save every frame (src/rendering.rs:110, :311): the `n_frames` RGB8 frames of
 * res_x x res_y pixels that the last render call left in the context's framebuffer (call it with rgb_out = NULL: the pixels
 * then never cross PCIe) are filtered (type 2, Up), Huffman-coded (one dynamic block per frame, distance-1 matches for zero
 * runs) and check-summed (Adler-32) by HIP kernels; what comes back is one finished zlib stream per frame, back to back in
 * `zlib_out` (host memory, preferably from curvis_host_alloc), frame f at [offsets[f], offsets[f + 1]) -- `offsets` has
 * n_frames + 1 entries.  curvis_image_save_zlib_rgb8 wraps such a stream into a PNG file (signature, IHDR, IDAT + CRC-32,
 * IEND: ~0.1 ms of a host thread per MB of stream instead of 4-7 ms per 1080p frame for filtering and coding on the
 * host).  CURVIS_E_INVALID with "output buffer too small" when out_cap does not suffice (worst case: 1.5 x the raw
 * frames + 200 bytes each; typical frames compress 10-100 x).  kernel_ms (may be NULL): HIP-event time of the launches. */
int curvis_ctx_deflate_frames(curvis_ctx *ctx, uint32_t res_x, uint32_t res_y, uint32_t n_frames, uint8_t *zlib_out, size_t out_cap,
                              size_t *offsets, double *kernel_ms);
int curvis_image_save_zlib_rgb8(const char *path, const uint8_t *zlib_stream, size_t len, uint32_t w, uint32_t h);
/* the same with the PNG chunk's CRC-32 from the device: idat_crc[f] = CRC-32 of "IDAT" + frame f's stream (Adler-32 trailer
 * included), *crc_valid = 1 on success (always, since round 6: one device path for every frame width; the flag stays in the
 * signature -- until round 5 frames whose rows were no multiple of 64 bytes left it 0 and idat_crc untouched).  curvis_image_save_zlib_rgb8_crc then writes the file without reading the stream again: what is left
 * to a writer thread is the write itself. */
int curvis_ctx_deflate_frames_crc(curvis_ctx *ctx, uint32_t res_x, uint32_t res_y, uint32_t n_frames, uint8_t *zlib_out, size_t out_cap,
                                  size_t *offsets, double *kernel_ms, uint32_t *idat_crc, int *crc_valid);
int curvis_image_save_zlib_rgb8_crc(const char *path, const uint8_t *zlib_stream, size_t len, uint32_t w, uint32_t h, uint32_t idat_crc);

/* Page-locked host memory for the `rgb_out` buffers of the render calls: into such a buffer the device-to-host copy of
 * a frame is ONE DMA transfer (~25 GB/s over PCIe 5), into ordinary pageable memory the runtime stages it through
 * bounce buffers (~2 GB/s measured: 12 ms of a 54 ms 4K frame).  `curvis video` keeps a small pool of these and hands
 * them to its PNG writer threads without another copy.  Free with curvis_host_free; no reference counterpart. */
int curvis_host_alloc(size_t bytes, void **out);
void curvis_host_free(void *p);

/* device framebuffer of the last render (RGB8, frames back to back) */
int curvis_ctx_framebuffer(curvis_ctx *ctx, void **dev_ptr, size_t *bytes);
int curvis_ctx_download(curvis_ctx *ctx, uint8_t *rgb_out, size_t bytes);
/* RGB8 frames from host memory into the context's framebuffer (frames back to back; it grows as needed): what
 * curvis_ctx_deflate_frames then compresses */
int curvis_ctx_upload(curvis_ctx *ctx, const uint8_t *rgb, size_t bytes);
int curvis_ctx_synchronize(curvis_ctx *ctx);
/* Overlapped stream download (option "async_streams" = 1, default 0): curvis_ctx_deflate_frames[_crc] returns while the frames'
 * zlib streams are still travelling to `zlib_out` on the context's copy stream.  Offsets, the Adler-32 trailers (written by the
 * host behind every stream: they need the sums, not the bytes) and the chunk CRCs are final on return; the stream bytes are
 * there after curvis_ctx_download_wait -- call it before anything reads `zlib_out`, e.g. after the NEXT render call has
 * returned, which is what the copy hides under (`curvis video`: one context 8 600 -> 10 600 frames/s).  The next deflate call
 * waits by itself before it reuses the scratch the streams are read from; so does switching the option off and
 * curvis_ctx_destroy.  `zlib_out` must stay valid until then (page-locked memory from curvis_host_alloc for a real overlap).
 * Read-only option "streams_pending". */

/* Overlapped download (option "async_download" = 1, default 0).  The reference's render_image returns an owned host
 * image (src/systems.rs:314-329), so a host that renders frame after frame pays the PCIe copy behind every kernel
 * (+0.25 ms on a 10.2 ms 1080p frame).  With the option set, a render call given `rgb_out` (brute, rows, batch, efficient,
 * direct) returns as soon as its kernels have finished and its statistics are valid, with the copy into `rgb_out` QUEUED
 * on a copy stream of the context; the next call renders into a second frame buffer while the copy engine drains the
 * first.  A pipeline one frame deep: `rgb_out` of call k is complete when call k + 1 with an `rgb_out` on the same
 * context returns, or when curvis_ctx_download_wait returns -- not before.  `rgb_out` should come from
 * curvis_host_alloc (into pageable memory the runtime's copy is not asynchronous; still correct).  Everything that reads
 * "the frames of the last render" (curvis_ctx_deflate_frames, curvis_ctx_download, curvis_ctx_framebuffer) keeps seeing them;
 * the device pointer curvis_ctx_framebuffer returns alternates between two buffers from call to call.  Setting the
 * option back to 0 waits for the download in flight, and so does curvis_ctx_destroy.  get_option: "downloads_overlapped"
 * (so far), "download_pending" (0 / 1). */
int curvis_ctx_download_wait(curvis_ctx *ctx);

/* tuning knobs (not part of the reference surface): "variant" (-1 = automatic, the default: the static
 * one-ray-per-thread kernel, and for launches of up to "relay_max_frames" (default 8) frames with at least "relay_min_blocks" workgroups
 * -- default 4 per CU, i.e. from about 700x400 -- the relay kernel; 0 = persistent lane-refill kernel;
 * 1 = static kernel always; 2 = relay kernel = the static kernel with end-game hand-over of unfinished tiles
 * between waves, still subject to "relay_min_blocks"; "relay_segment" = steps between hand-over points,
 * 0 = automatic; all variants give identical results), "block_threads" (workgroup size of the static / relay
 * kernels: 64, 128 or 256; 0 = automatic = 256), "refill_threshold",
 * "blocks_per_cu", "fast_math"
 * (1 = shared-reciprocal Euler step, 0 = compiler IEEE division/sqrt; identical results), "fuse_shade"
 * (1 = the static kernel shades in its epilogue, 0 = final states staged in HBM + separate shade kernel),
 * "supersample" (N = 1, 2, 4 or 8, default 1; anything else is refused with CURVIS_E_INVALID and the old value stays.  With N > 1
 * every render entry point -- brute, rows, batch, efficient, efficient batch, direct -- traces N x N rays per pixel of the cameras'
 * res_x x res_y and still returns res_x x res_y frames: with A the frame the same renderer gives at supersample = 1 for the same
 * cameras at N res_x x N res_y, out[y][x][c] = (sum of the 8-bit values A[N y + j][N x + i][c], i, j < N, + N^2 / 2) >> (2 log2 N);
 * the kernels average inside the wave that holds an 8x8 tile of the fine grid, which is why N divides 8.  Every counter --
 * curvis_stats, curvis_ctx_frame_stats, the sampler's records -- is that of the fine render, so rays = N^2 res_x res_y, also for
 * the efficient and direct renderers; a row band is given in output rows.  Framebuffer, downloads and the PNG front end see
 * res_x x res_y frames.  Refused with CURVIS_E_INVALID while N > 1: curvis_render_brute_debug (one record per ray),
 * "variant" = 0 and "fuse_shade" = 0 (rays staged one by one: no tile-local resolve)),
 * "sky_filter" (0 = nearest, the default and the reference's lookup bit for bit, or 1 = bilinear; anything else is refused with
 * CURVIS_E_INVALID "sky_filter must be 0 (nearest) or 1 (bilinear)" and the old value stays.  For a ray that escapes to a sky of
 * w x h RGBA8 texels T[y][x] with final direction d:
 *   1. (X, Y) are the raw `as u32` indices that the nearest lookup returns for a sky of 256 w x 256 h texels with the same
 *      orientation: its floating-point sequence with (double)(256 w) and (double)(256 h) in place of (double)w and (double)h and
 *      nothing else changed (the efficient renderer's instantiation with the call's reciprocals included).  Multiplying by a power
 *      of two commutes with rounding, so X >> 8 and Y >> 8 are the nearest lookup's raw tx and ty, bit for bit: the filter costs no
 *      additional FP64 operation, and the nearest texel of a filtered ray is the reference's.
 *   2. The ray is out of bounds exactly when X >> 8 >= w or Y >> 8 >= h -- the same rays as with the filter off, counted in n_oob
 *      as there.  Then Xc = min(X, 256 w - 1) and Yc = min(Y, 256 h - 1).
 *   3. Longitude wraps around the seam, with texel centres at 256 x + 128: U = Xc - 128 if Xc >= 128, else Xc + 256 w - 128;
 *      x0 = U >> 8, fx = U & 255, x1 = x0 + 1, or 0 when that equals w.
 *   4. Colatitude clamps at the poles: V = max(Yc - 128, 0); y0 = V >> 8, fy = V & 255, y1 = min(y0 + 1, h - 1).
 *   5. For each of R, G and B: out = ((256 - fx)(256 - fy) T[y0][x0] + fx (256 - fy) T[y0][x1] + (256 - fx) fy T[y1][x0]
 *      + fx fy T[y1][x1] + 32768) >> 16.  The weights are integers that sum to 65536, the whole expression fits 32 bits, and half
 *      rounds up; alpha is ignored.  (Not a two-stage lerp with intermediate rounding.)
 * Capped rays stay black, and all counters are those of the nearest render.  With "supersample" = N every sub-ray is filtered and
 * the N x N box average is taken over the filtered colours.  A render call with the filter on and a sky wider or taller than 2^23
 * texels fails with CURVIS_E_INVALID (256 w must stay a u32); so do, as under supersampling, curvis_render_brute_debug,
 * "variant" = 0 and "fuse_shade" = 0.  Sampler prefetch, PNG front end, downloads, row bands and batches are untouched),
 * "sky_mipmap" (0 = off, the default, or 1; anything else is refused with CURVIS_E_INVALID and the old value stays.  It acts on top of
 * the bilinear filter: setting it is always allowed, in either order with "sky_filter", and a render call with "sky_mipmap" = 1 and
 * "sky_filter" = 0 fails with CURVIS_E_INVALID.  With 0 nothing changes.  With 1:
 *   Pyramid.  Level 0 is the sky T0 of w x h texels.  Level k+1 has w_{k+1} = (w_k + 1) >> 1 by h_{k+1} = (h_k + 1) >> 1 texels, and
 *     T_{k+1}[y][x] is, per colour channel, (a + b + c + d + 2) >> 2 of the four values of level k at columns 2x and
 *     min(2x + 1, w_k - 1), rows 2y and min(2y + 1, h_k - 1); alpha is 255.  One rounding per level, half up.  There are
 *     L = 1 + ceil(log2(max(w, h))) levels, the last of 1 x 1.  Where a size is odd the last column or row counts its source twice:
 *     the definition is this recurrence, not an area average.
 *   Footprint.  Rays are paired in 2 x 2 quads of absolute ray coordinates: the partners of ray (px, py) are (px ^ 1, py) and
 *     (px, py ^ 1) -- coordinates of the fine grid under "supersample", of the frame (not of the band) in a row band.  For a ray that
 *     escaped to sky s, with the (Xc, Yc) of step 2 of "sky_filter", each partner contributes dX = |wrap(Xc' - Xc)|, where wrap
 *     reduces modulo 256 w into [-128 w, 128 w), and dY = |Yc' - Yc|; a partner outside the frame, capped (black) or escaped to the
 *     other sky contributes nothing.  rho is the largest of the up to four contributions, 0 without any.
 *   Level.  rho < 256: k = 0, f = 0.  Otherwise k = msb(rho) - 8 and f = (rho >> k) & 255.  Then, if k >= L - 1: k = L - 1, f = 0
 *     (a render never gets there, since rho <= max(128 w, 256 h - 1); it makes the function total).
 *   Colour.  c_k is steps 3-5 of "sky_filter" applied to T_k with w_k, h_k, X_k = Xc >> k and Y_k = Yc >> k (X_k < 256 w_k always
 *     holds); level 0 is the "sky_filter" = 1 colour bit for bit.  f = 0: the colour is c_k.  Otherwise, per channel,
 *     out = ((256 - f) c_k + f c_{k+1} + 128) >> 8.
 * Counters, n_oob, the nearest lookup's tx and ty are unchanged, capped rays stay black, and the "supersample" box average is taken
 * over the mip-filtered sub-ray colours.  Row bands: so that the quads do not depend on how a frame is split, a band of
 * curvis_render_brute_rows must, in rows of the ray grid, begin on an even row and hold an even number of rows unless it ends on the
 * frame's last row; otherwise the call fails with CURVIS_E_INVALID (with "supersample" > 1 every band of output rows qualifies).
 * Refused with CURVIS_E_INVALID while it is 1, as under "sky_filter": curvis_render_brute_debug, "variant" = 0 and "fuse_shade" = 0.
 * The levels above 0 (a third of the sky's bytes) belong to the context's sky; they are built on the context's stream by the first
 * render call with the option on -- a context that never sets it allocates nothing -- and dropped by curvis_ctx_set_sky,
 * curvis_ctx_set_sky_device and curvis_ctx_bcast_skies (every device rebuilds its own chain).  The relay kernel is not used while the
 * option is on),
 * "projection" (0 = perspective, the default and the reference's mapping bit for bit, 1 = equirectangular, 2 = equidistant fisheye;
 * anything else is refused with CURVIS_E_INVALID and the old value stays.  It replaces only the three expressions that form the
 * un-normalised camera-space vector vec = (x, y, z) of a pixel (camera axes as in the reference: x forward, y left, z up); everything
 * behind it is the reference's sequence unchanged -- vec.normalize() with norm sqrt((x x + y y) + z z) and three divisions, the camera
 * rotation, new_photon's second normalisation, the Euler loop and the lookup; in the efficient and direct renderers rot_bg, the
 * cross product and acos.  Every operation is an individually rounded FP64 one in the order written, no contraction; sin and cos
 * are cv_math.h's table-driven ones, pi is CV_PI and 2 pi is 2.0 * CV_PI.  For projection != 0 a pixel is sampled at its centre:
 *   u = (double)(2 px + 1) / (double)(2 res_x),  v = (double)(2 py + 1) / (double)(2 res_y)
 * each ONE correctly rounded quotient of two exactly representable integers (the efficient pixel kernel forms it from the call's
 * shared reciprocals and delivers that quotient).
 *   1, equirectangular (focal, sensor_w, sensor_h are not read):
 *      psi = (0.5 - u) * (2 pi),  th = v * pi,  vec = (sin(th) cos(psi), sin(th) sin(psi), cos(th))
 *      -- the image centre looks along `forward`, the left and right edges meet looking backward, row 0 is nearest `up`.
 *   2, fisheye (image radius = focal * angle from the axis, on the camera's own sensor and focal length):
 *      ys = -sensor_w * (u - 0.5),  zs = sensor_h * (0.5 - v),  rho = sqrt(ys ys + zs zs),  b = rho / focal,
 *      vec = (cos(b), sin(b) (ys / rho), sin(b) (zs / rho)), and vec = (1, 0, 0) when rho == 0 (the centre pixel of an odd x odd
 *      frame).  A render call fails with CURVIS_E_INVALID when 0.5 sqrt(sensor_w^2 + sensor_h^2) / focal > pi.
 * With "supersample" = N, px, py, res_x, res_y are the fine grid's and the box average is that of the frame the same renderer
 * gives at N res_x x N res_y; "sky_filter" acts on the final direction and is untouched; counters are those of the rays actually
 * traced.  Refused with CURVIS_E_INVALID while projection != 0, as under the two options above: curvis_render_brute_debug,
 * "variant" = 0 and "fuse_shade" = 0 (only the fused kernels have the projections).  The relay seat belt checks a projected launch
 * shape on its own),
 * "step_scale" (an integer S, 0 <= S <= 2^20, default 0 = off: every Euler step takes the call's delta, the reference's loop bit for
 * bit and the kernels that exist without the option; anything else is refused with CURVIS_E_INVALID and the old value stays.  For
 * S != 0 and a render call with step delta:
 *   1. L0 = (double)S / 256.0 (exact): the coordinate distance inside which the step is the reference's.
 *   2. kappa = RN(delta / L0), formed once per call on the host with one IEEE double division.
 *   3. Step k of a ray whose radial coordinate BEFORE the step is l_k uses a = RN(|l_k| kappa) and delta_k = (a > delta) ? a : delta;
 *      a NaN l_k therefore gives delta.  (The code, cv_device.h step_delta, forms it as the IEEE maximum fmax(a, delta): the same value for
 *      every input a render call admits -- a > delta gives a, a <= delta gives delta, and for a NaN a the maximum returns its other
 *      operand, delta, which is a number because delta > 0 is checked on the host -- and one instruction on the device.)
 *   4. The step itself is the reference's update_relativistic_object with delta_k in place of delta: operations, order and roundings
 *      are otherwise unchanged, and the fast step keeps its contract (correctly rounded quotients).
 *   5. The escape test after each step, the max_iterations cap counted in steps, new_photon, direction, lookup and every counter
 *      are unchanged; `steps` counts executed steps, so it becomes smaller.
 *   6. In the debug dump x[0] follows the reference's line with the same delta_k: t_{k+1} = t_k + (1.0 * -1.0) * delta_k.
 * All three renderers honour it (the efficient renderer in both samplers; its per-pixel kernel never integrates); it combines with
 * "supersample", "sky_filter" and "projection", row bands, batches and the prefetch, whose jobs it is part of.  With S != 0 the brute
 * renderer launches the static kernel, never the relay kernel.  A render call with S != 0 and !(delta > 0) fails with
 * CURVIS_E_INVALID; so do, while S != 0, "fast_math" = 0 (every renderer), "variant" = 0 and, outside the debug dump,
 * "fuse_shade" = 0.  curvis_render_brute_debug is served (when none of the three options above is on).
 * curvis_photon_trajectories, curvis_compute_escape_angles and curvis_update_relativistic_object take their delta explicitly and
 * do not look at the option; curvis_step_delta evaluates step 3 on the host),
 * "integrator" (0, the default: forward Euler, the reference's loop bit for bit and the kernels that exist without the option; 1: Heun's
 * method, the explicit trapezoid, second order; anything else is refused with CURVIS_E_INVALID and the old value stays.  With E(y, d)
 * the reference's update_relativistic_object, y + d/2 (f(y) + f(y + d f(y))) = 1/2 (y + E(E(y, d), d)), so for integrator = 1 step k of
 * a ray in state y_k = (l, theta, phi, p_l, p_theta):
 *   1. delta_k is what "step_scale" defines from l_k, the radial coordinate before the step: step_delta(delta, kappa, l_k); with
 *      "step_scale" = 0 it is delta.  (The code runs one path for both: with kappa = +0, |l| kappa is 0 or NaN and the maximum with
 *      delta > 0 is delta, for every l.)
 *   2. y' = E(y_k, delta_k) and y'' = E(y', delta_k): the reference's step, every operation individually rounded in its order -- in
 *      the kernels the fast step under its contract.  Both stages use the same delta_k; the scale is not re-evaluated at y'.
 *   3. y_{k+1}[c] = (y_k[c] + y''[c]) * 0.5 for c in {l, theta, p_l, p_theta}, and phi where it is integrated: one IEEE add, then one
 *      IEEE multiply.  p_phi (and p_t) are constants of the step and are kept, not averaged.  The debug dump's x[0] is averaged the
 *      same way over t'' = (t + (1.0 * -1.0) delta_k) + (1.0 * -1.0) delta_k.
 *   4. The escape test |l| > max_radius is made on y_{k+1} only, never on a stage.  max_iterations and the counter `steps` count Heun
 *      steps; each is two evaluations of the right-hand side.  new_photon, direction, lookup and the other counters are unchanged.
 * All three renderers honour it (the efficient renderer in both samplers); it combines with "step_scale", "supersample",
 * "sky_filter" and "projection", row bands, batches and the prefetch, whose jobs it is part of.  With integrator = 1 the brute
 * renderer launches the static kernel, never the relay kernel.  Refused with CURVIS_E_INVALID while integrator = 1, as under
 * "step_scale": a render call with !(delta > 0), "fast_math" = 0 (every renderer), "variant" = 0 and, outside the debug dump,
 * "fuse_shade" = 0.  curvis_render_brute_debug is served.  curvis_photon_trajectories, curvis_compute_escape_angles and
 * curvis_update_relativistic_object stay the reference's functions; curvis_heun_step evaluates steps 2 and 3 on the host),
 * "max_store_bytes" (ray-store budget that bounds the frames per launch of a batch),
 * "sampling_speculation" (efficient renderer: depth of the speculative dyadic subtree evaluated below every
 * refined interval; 0 = one launch per refinement round; default -1 = automatic, 10 for one or two frames, 6 for three to five and 4
 * for larger batches) and "sampling_speculation_first" (the same below the intervals of the initial uniform grid,
 * i.e. for the first launch; default -1 = automatic, 8 / 4 / 3; depths up to 11), "device_sampler" (efficient renderer: 1 = the
 * reference's whole adaptive sampler -- rounds, speculation and all -- runs on the device, ONE launch per call and a workgroup
 * per distinct camera radius, no host in the refinement loop; 0 = the host-paced sampler, several launches per call; default -1 =
 * automatic: the device from "device_sampler_min_frames" (default 48) frames per call on; identical sample tables and pixels either
 * way; a table that outgrows the kernel's fixed arrays -- 1536 samples -- sends the call to the host-paced sampler;
 * "sampling_speculation" = 0 switches speculation off on the device too); read-only after an efficient render:
 * "last_sampling_launches", "last_sampling_evaluated", "last_sampler_path" (0 host-paced, 1 device, 2 device fell back to the
 * host), "last_sampling_chains" (device: Euler chains the slowest job waited for), "last_pixel_tiled" (1 when the per-pixel launch
 * enumerated pixels by 8x8 tiles -- "supersample" > 1, "sky_mipmap" = 1, or the measurement switch "pixel_tiled" = 1, which asks for
 * that enumeration where the linear kernel would do: same frames, same counters --, else 0); after a mip chain build:
 * "last_sky_mip_build_us" (HIP-event time of its launches), after curvis_ctx_set_sky_device with copy != 0: "last_sky_copy_us"; after any render: "last_frames"; after a relay render: "last_relay_launches",
 * "last_relay_parks".  Relay safety net: if a relay launch reports waves that gave up waiting (the kernel leans
 * on in-order workgroup dispatch, which HIP does not promise), the frame is rendered again by the static kernel and
 * "relay_disabled" becomes 1 for the context ("relay_fallbacks" counts such renders); "relay_verify" = 1 (debug)
 * repeats every relay render with the static kernel and fails with CURVIS_E_HIP if frames or counters differ. */
int curvis_ctx_set_option(curvis_ctx *ctx, const char *key, int64_t value);
int curvis_ctx_get_option(const curvis_ctx *ctx, const char *key, int64_t *value);

/* self-test hooks used by tests/ (device vs host bit-equality of cv_math.h and of IEEE div/sqrt):
 * op: 0 sin, 1 cos, 2 atan, 3 acos, 4 log, 5 atan2(a,b), 6 a/b, 7 sqrt(a), 8 fma(a,b,a),
 * 9 raw v_rcp_f64(a), 10 raw v_rsq_f64(a) (hardware seeds, for accuracy measurements) */
int curvis_selftest_math(curvis_ctx *ctx, int op, const double *a, const double *b, double *out, size_t n);

/* the primitives of the shared-reciprocal Euler step, element-wise on three inputs (b, c may be NULL where unused):
 * op 0 div_with_recip(n = a, d = b, y = c): the quotient the fast step forms from an approximate reciprocal y
 *    1 sqrt_and_rsqrt(a): the square root    2 sqrt_and_rsqrt(a): its by-product y ~ 1/sqrt(a)
 *    3 the square root's final residual step for given (x, g, y) = (a, b, c)
 *    4 recip_refined(a)    5 cv_div_nr(a, b) (the -1/x of atan)    6 recip_newton(d = a, y = b)
 *    7 / 8 / 9 component 0 / 1 / 2 of v / |v| for v = (a, b, c) through the efficient pixel kernel's shared reciprocal (unit3)
 *    10 a / b as the pixel kernel divides an index by a constant (div_index, y = recip_chain(b))    11 ... an angle (div_angle)
 *    12 sqrt(a) through the pixel kernel's sqrt_plain (the compiler's chain without its range wrappers)
 *    13 Rust's `a as u32` (saturating, NaN -> 0) as the sky lookup converts its texel coordinates
 * -- the directed hard cases of tests/test_gpu_fast_step.py go through here. */
int curvis_selftest_math3(curvis_ctx *ctx, int op, const double *a, const double *b, const double *c, double *out, size_t n);

/* ONE Euler step (src/metrics.rs:283-297) of the fast kernel per input state, every quotient recorded.
 * states: n x {l, theta, p_l, p_theta, p_phi}; out: n x CURVIS_FAST_STEP_RECORD doubles =
 *   6 x {numerator n, denominator d, shared reciprocal y used, the step's quotient, the IEEE quotient, the remainder
 *        n - d RN(n y), 1 - d y}
 *       (k = 0 r' = l/r [Ellis only], 1 1/r^2, 2 p_phi^2/sin^2, 3 dp_l, 4 cos/(r^2 sin^3), 5 1/(r^2 sin^2); NaN = not formed),
 *   5 new state of the fast step (l, theta, phi - phi0, p_l, p_theta), 5 of the strict step, 1 flag (1 = fast path taken). */
#define CURVIS_FAST_STEP_RECORD 53
int curvis_selftest_fast_step(curvis_ctx *ctx, const curvis_metric *metric, double delta, double max_radius, const double *states,
                              size_t n, double *out);

/* the sky lookup (direction -> texel indices, src/images.rs:115-174) as the kernels compile it, on chosen directions: a sky of
 * w x h texels with inverse rotation inv_rot (row-major 3 x 3; no image is needed), dirs = n x {d0, d1, d2};
 * out: n x {tx, ty as the brute and direct renderers compute them, tx, ty as the efficient renderer's per-pixel kernel does, with
 * theta / pi and phi / 2 pi through the shared reciprocals an efficient render call of this context uses} -- raw `as u32`
 * values, BEFORE the clamp to w - 1 / h - 1 (ty == h for a direction on the -z axis).  tests/test_gpu_sky_lookup.py. */
int curvis_selftest_sky_indices(curvis_ctx *ctx, uint32_t w, uint32_t h, const double inv_rot[9], const double *dirs, size_t n,
                                uint32_t *out);

/* the filtered lookup of option "sky_filter" = 1 as the kernels compile it, on chosen directions: rgba is a HOST image of w x h
 * RGBA8 texels (w * h * 4 bytes), dirs = n x {d0, d1, d2}; out_taps: n x 2 x {x0, x1, y0, y1, fx, fy}, out_rgb: n x 2 x {r, g, b} --
 * first as the brute and direct renderers compute them, then as the efficient renderer's per-pixel kernel does (shared
 * reciprocals, as in curvis_selftest_sky_indices).  tests/test_gpu_sky_filter.py. */
int curvis_selftest_sky_bilinear(curvis_ctx *ctx, uint32_t w, uint32_t h, const double inv_rot[9], const uint8_t *rgba, const double *dirs,
                                 size_t n, uint32_t *out_taps, uint8_t *out_rgb);

/* the per-ray colour of option "sky_mipmap" = 1 as the kernels compile it: rgba is a HOST image of w x h RGBA8 texels, whose mip chain
 * is built on the device; triples = n x {Xc, Yc, rho} (Xc, Yc beyond the virtual sky are clamped into it); out_rgb: n x {r, g, b}.  The
 * function has no floating-point part, so there is one instantiation.  tests/test_gpu_sky_mipmap.py. */
int curvis_selftest_sky_mip(curvis_ctx *ctx, uint32_t w, uint32_t h, const uint8_t *rgba, const uint32_t *triples, size_t n, uint8_t *out_rgb);

#ifdef __cplusplus
}
#endif
#endif /* CURVIS_HIP_H */
