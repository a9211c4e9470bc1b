/* curvis_hip.hip -- the ONE translation unit of libcurvis_hip.so (C ABI: include/curvis_hip.h), gfx950 only.
 *
 * Pieces (each included here and nowhere else; `make asm` before/after the split: the same instructions):
 *   kernels_epilogue.h   what the render kernels share behind their loops: per-frame counters and a wave's reduction into them,
 *                        direction -> colour (sky_lookup_bilinear, shade_ray's sky_lookup), colour -> frame buffer (store_rgb8, resolve_store)
 *   kernels_geodesic.h   device side of RelativisticSystem::render_image (src/systems.rs:307-330, rows R1-R10 of SURVEY.md 8a)
 *   kernels_efficient.h  device side of render_image_efficient (src/systems.rs:333-527), direct mode, trajectories, math self-test
 *   hip_owned.h          the owners of the HIP resources (device / page-locked buffers, events, streams, sky textures): what a
 *                        context or a call holds is freed by destructors, on every return path
 *   render_host.h        struct curvis_ctx, with_kind / with_flag (metric kind and step flavour -> template arguments) and
 *                        with_launch_shape (those two, supersample, sky_filter and projection -> one tag type), prepare_call_shape
 *                        (what the three options make of a call, for all three renderers), launch_integrate (the one launch of the
 *                        kernel family the plan names), render_impl = facts of the call + render_chunk + relay_seat_belt, per-frame statistics
 *   brute_plan.h         host only, plain C++ (g++ compiles it alone): from the facts of a brute call to its plan -- the refusals as a
 *                        table, fused / relay, the kernel family -- and the launch shapes each family is instantiated for
 *   efficient_host.h     the adaptive sampler's driver (src/sampling.rs) over batched escape-angle launches, the device sampler's
 *                        slots and prefetch, per-pixel launch and statistics shared by the two
 *   kernels_png.h, png_host.h   PNG front end on the device: the frames in HBM -> one zlib stream per frame (src/rendering.rs:110, :311)
 *   (this file)          the extern "C" entry points; kOptions, the one table of option keys behind set_option / get_option
 *   per-ray arithmetic: cv_device.h / cv_efficient.h / cv_sampler.h / cv_math.h (shared with the host twin of the tests)
 *
 * Kernels
 *   geodesic_relay<KIND,FAST>              DEFAULT for launches of <= 8 frames that fill the chip (>= 4 workgroups per CU):
 *       the static kernel's loop in segments; in the end-game of a launch unfinished 8x8 tiles are parked in HBM (40 B per
 *       ray, write-through) and picked up by relay workgroups the dispatcher places wherever slots are free.
 *   geodesic_static<KIND,PHI,FAST,FUSED>   default for larger batches, small frames and the debug dump, and the relay
 *       kernel's checker: one ray per lane -- pixel -> photon -> forward-Euler loop to escape or cap with a wave-uniform
 *       step counter -> (FUSED) tangent direction, nearest sky texel, RGB8 store in the epilogue, i.e. R1-R10 in ONE
 *       launch per batch of frames and no intermediate HBM traffic.  Hardware block scheduling balances the grid.
 *   geodesic_persistent<KIND,PHI,FAST>     persistent waves: when `refill_threshold` lanes of a wave have terminated they
 *       are stored together and the free lanes are refilled from a global ray queue with ONE wave-aggregated atomic
 *       (ballot + popcount + mbcnt rank).  Final states are staged in the ray store and shaded by shade_kernel.
 *       Selectable ("variant" = 0); measured 3-8 % slower than the static kernel on every workload tried.
 *   shade_kernel<KIND,DEBUG>               staged shading (persistent kernel, debug dump of every ray).
 *   escape_angle_kernel<KIND,FAST>, efficient_pixel_kernel, direct_kernel, trajectory_kernel   efficient mode and extras.
 *   geodesic_static / geodesic_relay / direct_kernel<..., SS>, efficient_pixel_ss_kernel<SS>   option "supersample" = SS in
 *       {2, 4, 8} (SS = 1: the kernels above): the same kernels over the SS times finer ray grid; the wave that holds an 8x8 tile of it averages every SS x SS
 *       block across its lanes (DPP / ds_swizzle / ds_bpermute) and stores one pixel per block (kernels_epilogue.h resolve_store).
 *   the same with a trailing FILTER = 1 (efficient_pixel_kernel<1>, efficient_pixel_ss_kernel<SS, 1>)   option "sky_filter" = 1: the
 *       epilogues blend the four texels around the direction (cv_device.h sky_bilinear_taps / sky_bilinear_blend) instead of
 *       fetching the nearest; FILTER = 0 are the kernels above, instruction for instruction.
 *   the same with a trailing PROJ = 1      option "projection" != 0: the prologues form the pixel's camera-space vector by
 *       cv_device.h camera_pixel_vector's equirectangular or fisheye branch (a scalar branch on a kernel argument; nothing of it
 *       lives into the Euler loop); PROJ = 0 are the kernels above, instruction for instruction.
 *   the same with FILTER = 2 (geodesic_static, direct_kernel, efficient_pixel_ss_kernel<SS, 2> with SS = 1 included; no relay form)
 *       option "sky_mipmap" = 1 on top of the filter: the wave exchanges every ray's sky indices inside its 2 x 2 quads and each lane
 *       blends two levels of the sky's mip chain (kernels_epilogue.h sky_mip_shade); the argument is the FILTER = 1 kernel's with the
 *       level tables appended.
 *   efficient_pixel_ss_kernel<1, FILTER>   FILTER = 0, 1: the tile enumeration alone, reached through option "pixel_tiled" = 1 only
 *       (tools/gpu_sky_mipmap_cost.py times it beside the linear kernel).
 *   sky_mip_kernel                         one level of a sky's mip chain from the level below it.
 *   selftest_sky_mip_kernel                the per-ray colour of "sky_mipmap" on the tests' (Xc, Yc, rho).
 *   selftest_sky_bilinear_kernel           the two functions alone, both instantiations, on the tests' directions.
 *   selftest_math_kernel                   cv_math.h / IEEE div / sqrt / hardware seeds for the tests.
 *   selftest_sky_indices_kernel            cvk::sky_indices (direction -> texel), both instantiations, on the tests' directions.
 *   FAST = shared-reciprocal Euler step (cv_device.h ray_step_fast), !FAST = compiler IEEE div/sqrt;
 *   PHI = integrate phi as well (debug dump, escape angles).
 *
 * Ray order: rays are numbered by 8x8 pixel tiles (tile-major, then row-major inside the tile) so the 64 rays of a wave
 * are spatial neighbours: similar step counts, neighbouring sky texels, 3-byte stores that cover whole 24-byte row segments.
 *
 * No MFMA (nothing here is a contraction).  Ray state lives in registers (5 doubles per ray); LDS holds the read-only
 * function tables of cv_math.h (8 KiB Ellis, 28 KiB Interstellar per workgroup).  The loop is an issue-bound chain of FP64
 * VALU ops (5 divisions, sqrt, sincos per step); HBM traffic is 3 B out + 4 B in per ~2000 steps.
 */
#include <hip/hip_runtime.h>
#include <dirent.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <atomic>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/curvis_hip.h"
#include "cv_device.h"
#include "cv_efficient.h"
#include "cv_frame_host.h"
#include "cv_host.h"
#include "cv_sampler.h"
#include "cv_sampler_dev.h"
#include "host/jpeg_io.h" /* PNG + JPEG decoders shared with the curvis binary */

#pragma clang fp contract(off)

#include "kernels_epilogue.h"
#include "kernels_geodesic.h"
#include "kernels_efficient.h"
#include "hip_owned.h"
#include "brute_plan.h"
#include "render_host.h"
#include "efficient_host.h"
#include "png_codes.h"
#include "kernels_png.h"
#include "png_host.h"

/* ------------------------------------------------------------------------------------------ ABI */
extern "C" {

const char *curvis_version(void) { return "curvis_amd 0.1 (gfx950, abi 1)"; }

const char *curvis_last_error(const curvis_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int curvis_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int curvis_ctx_create(int device, curvis_ctx **out) {
  if (!out) return fail(nullptr, CURVIS_E_INVALID, "out is null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, CURVIS_E_NO_DEVICE,
                "no HIP device visible: libcurvis_hip has no CPU fallback (hipGetDeviceCount: " +
                    std::string(hipGetErrorString(e)) + ")");
  if (device < 0 || device >= n) return fail(nullptr, CURVIS_E_NO_DEVICE, "device index out of range");
  curvis_ctx *ctx = new curvis_ctx();
  ctx->device = device;
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < 9; ++i) ctx->sky_inv_rot[s][i] = (i % 4 == 0) ? 1.0 : 0.0;
  auto bail = [&](int code, const std::string &m) {
    g_create_error = m;
    curvis_ctx_destroy(ctx);
    return code;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(CURVIS_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  if ((e = hipGetDeviceProperties(&ctx->prop, device)) != hipSuccess)
    return bail(CURVIS_E_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
  if (std::strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0)
    return bail(CURVIS_E_NO_DEVICE, std::string("device is ") + ctx->prop.gcnArchName + ", this library carries gfx950 code only");
  if (ctx->stream.ensure(ctx, hipStreamNonBlocking) || ctx->ev0.ensure(ctx) || ctx->ev1.ensure(ctx) || ctx->ev2.ensure(ctx))
    return bail(CURVIS_E_HIP, std::string(ctx->err)); /* (a copy: bail deletes the context) */
  *out = ctx;
  return CURVIS_OK;
}

void curvis_ctx_destroy(curvis_ctx *ctx) {
  if (!ctx) return;
  if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
  /* these three waits are what makes the order in which the members' destructors free things immaterial: nothing is in flight */
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream); /* a download still in flight reads d_fb / d_fb_alt */
  if (ctx->sampler_stream) (void)hipStreamSynchronize(ctx->sampler_stream); /* a prefetched sampler still writes its slot */
  delete ctx;
}

int curvis_ctx_device_info(const curvis_ctx *ctx, char *name, size_t name_cap, int *compute_units, int *clock_mhz) {
  if (!ctx) return CURVIS_E_INVALID;
  if (name && name_cap) {
    /* some hosts' driver stack reports no marketing name (hipDeviceProp_t::name empty: no amdgpu.ids entry): take the
     * board's product name from sysfs then, and say so rather than print nothing */
    std::string nm = ctx->prop.name;
    if (nm.find_first_not_of(' ') == std::string::npos) {
      char id[64] = {0};
      if (hipDeviceGetPCIBusId(id, (int)sizeof id, ctx->device) == hipSuccess) {
        for (char *p = id; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
        if (FILE *f = std::fopen((std::string("/sys/bus/pci/devices/") + id + "/product_name").c_str(), "r")) {
          char line[128] = {0};
          if (std::fgets(line, sizeof line, f)) nm = line;
          std::fclose(f);
          while (!nm.empty() && (nm.back() == '\n' || nm.back() == ' ')) nm.pop_back();
        }
      }
      if (nm.find_first_not_of(' ') == std::string::npos) nm = "AMD GPU, name not reported by the driver";
    }
    std::snprintf(name, name_cap, "%s (%s)", nm.c_str(), ctx->prop.gcnArchName);
  }
  if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
  if (clock_mhz) *clock_mhz = ctx->prop.clockRate / 1000;
  return CURVIS_OK;
}

/* first integer of a small sysfs file matched by `glob`-less path pieces; -1 when unreadable */
static long read_sysfs_long(const std::string &path) {
  FILE *f = std::fopen(path.c_str(), "r");
  if (!f) return -1;
  long v = -1;
  if (std::fscanf(f, "%ld", &v) != 1) v = -1;
  std::fclose(f);
  return v;
}

int curvis_ctx_device_status(const curvis_ctx *ctx, char *pci_bus_id, size_t cap, int *sclk_mhz, int *power_w) {
  if (!ctx) return CURVIS_E_INVALID;
  char id[64] = {0};
  if (hipDeviceGetPCIBusId(id, (int)sizeof id, ctx->device) != hipSuccess) id[0] = 0;
  for (char *p = id; *p; ++p) *p = (char)std::tolower((unsigned char)*p); /* sysfs spells the address in lower case */
  if (pci_bus_id && cap) std::snprintf(pci_bus_id, cap, "%s", id);
  const std::string dev = std::string("/sys/bus/pci/devices/") + id;
  if (sclk_mhz) { /* pp_dpm_sclk: one line per level, "1: 2100Mhz *" marks the current one */
    *sclk_mhz = -1;
    if (FILE *f = std::fopen((dev + "/pp_dpm_sclk").c_str(), "r")) {
      char line[128];
      while (std::fgets(line, sizeof line, f)) {
        int level = 0, mhz = 0;
        if (std::strchr(line, '*') && std::sscanf(line, "%d: %dMhz", &level, &mhz) == 2) *sclk_mhz = mhz;
      }
      std::fclose(f);
    }
  }
  if (power_w) { /* hwmon/hwmonN/power1_average (or power1_input), microwatts */
    *power_w = -1;
    if (DIR *dir = opendir((dev + "/hwmon").c_str())) {
      while (struct dirent *e = readdir(dir)) {
        if (std::strncmp(e->d_name, "hwmon", 5) != 0) continue;
        const std::string h = dev + "/hwmon/" + e->d_name;
        long uw = read_sysfs_long(h + "/power1_average");
        if (uw < 0) uw = read_sysfs_long(h + "/power1_input");
        if (uw >= 0) {
          *power_w = (int)(uw / 1000000);
          break;
        }
      }
      closedir(dir);
    }
  }
  return CURVIS_OK;
}

static int set_sky_common(curvis_ctx *ctx, int which, uint32_t w, uint32_t h) {
  if (!ctx) return CURVIS_E_INVALID;
  if (which < 0 || which > 1) return fail(ctx, CURVIS_E_INVALID, "which must be 0 (+l) or 1 (-l)");
  if (w == 0 || h == 0) return fail(ctx, CURVIS_E_INVALID, "empty sky image");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return ctx->sky[which].reset(ctx, w, h);
}

int curvis_ctx_set_sky(curvis_ctx *ctx, int which, const uint8_t *rgba, uint32_t w, uint32_t h) {
  int rc = set_sky_common(ctx, which, w, h);
  if (rc) return rc;
  SkyTexture &S = ctx->sky[which];
  if ((rc = S.allocate(ctx))) return rc;
  if (rgba) {
    HIP_TRY(ctx, hipMemcpyAsync(S.texels, rgba, S.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CURVIS_OK;
}

int curvis_ctx_set_sky_device(curvis_ctx *ctx, int which, const void *dev_rgba, uint32_t w, uint32_t h, int copy) {
  if (!dev_rgba) return fail(ctx, CURVIS_E_INVALID, "null device pointer");
  int rc = set_sky_common(ctx, which, w, h);
  if (rc) return rc;
  SkyTexture &S = ctx->sky[which];
  if (!copy) {
    S.borrow(dev_rgba);
    return CURVIS_OK;
  }
  if ((rc = S.allocate(ctx))) return rc;
  if ((rc = ctx->ev0.ensure(ctx)) || (rc = ctx->ev1.ensure(ctx))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream)); /* the copy alone, by HIP events: option "last_sky_copy_us" */
  HIP_TRY(ctx, hipMemcpyAsync(S.texels, dev_rgba, S.bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last_sky_copy_us = (int64_t)(ms * 1000.0f + 0.5f);
  return CURVIS_OK;
}

int curvis_ctx_set_sky_orientation(curvis_ctx *ctx, int which, const double forward[3], const double up[3]) {
  if (!ctx || !forward || !up || which < 0 || which > 1) return fail(ctx, CURVIS_E_INVALID, "bad argument");
  cvh::Orientation o;
  if (!cvh::orientation_new(cvh::Vec3{forward[0], forward[1], forward[2]}, cvh::Vec3{up[0], up[1], up[2]}, o))
    return fail(ctx, CURVIS_E_PARALLEL, "Forward and up vectors must not be parallel (src/algebra.rs:19-21)");
  for (int i = 0; i < 9; ++i) ctx->sky_inv_rot[which][i] = o.inverse_rotation.m[i];
  return CURVIS_OK;
}

int curvis_ctx_set_disc(curvis_ctx *ctx, const uint8_t *rgba, uint32_t w, uint32_t h, double l_inner, double l_outer) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!rgba) { /* remove the disc: every call launches the kernels it launched before one was set */
    ctx->disc_set = false;
    return CURVIS_OK;
  }
  if (w == 0 || h == 0) return fail(ctx, CURVIS_E_INVALID, "disc: empty texture");
  if (!std::isfinite(l_inner) || !std::isfinite(l_outer)) return fail(ctx, CURVIS_E_INVALID, "disc: l_inner and l_outer must be finite");
  if (!(l_inner < l_outer)) return fail(ctx, CURVIS_E_INVALID, "disc: l_inner must be less than l_outer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* nothing in flight reads the texture that reserve may free */
  ctx->disc_set = false;
  if (int rc = ctx->d_disc.reserve(ctx, (size_t)w * h)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_disc, rgba, (size_t)w * h * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->disc_w = w, ctx->disc_h = h;
  ctx->disc_l_in = l_inner, ctx->disc_l_out = l_outer;
  ctx->disc_set = true;
  return CURVIS_OK;
}

int curvis_disc_crossing(double c_prev, double c_cur, double s_cur, double l_prev, double l_cur, double phi_prev, double phi_cur,
                         double l_inner, double l_outer, uint32_t w, uint32_t h, int32_t *hit, uint32_t *tx, uint32_t *ty) {
  if (!hit || !tx || !ty || w == 0 || h == 0) return CURVIS_E_INVALID;
  unsigned x = 0, y = 0;
  *hit = cvk::disc_crossing(c_prev, c_cur, s_cur, l_prev, l_cur, phi_prev, phi_cur, l_inner, l_outer, w, h, &x, &y) ? 1 : 0;
  *tx = x, *ty = y;
  return CURVIS_OK;
}

/* what RCCL itself has to say about a failure: the result's text, the communicator's last error, an asynchronous error */
static std::string rccl_detail(ncclComm_t comm, ncclResult_t rc) {
  std::string m = ncclGetErrorString(rc);
  const char *last = ncclGetLastError(comm);
  if (last && *last) m += std::string("; last RCCL error: ") + last;
  ncclResult_t async = ncclSuccess;
  if (comm && ncclCommGetAsyncError(comm, &async) == ncclSuccess && async != ncclSuccess)
    m += std::string("; asynchronous: ") + ncclGetErrorString(async);
  return m;
}
/* stream synchronisation of one stage of the broadcast, with the stage's name in the error (first contact between two
 * devices must say WHERE it broke: a collective's enqueue succeeds, its failure shows at the synchronisation) */
static int bcast_stage_sync(curvis_ctx *ctx, ncclComm_t comm, const char *stage) {
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  ncclResult_t async = ncclSuccess;
  (void)ncclCommGetAsyncError(comm, &async);
  if (e != hipSuccess || async != ncclSuccess)
    return fail(ctx, e != hipSuccess ? CURVIS_E_HIP : CURVIS_E_RCCL,
                std::string("sky broadcast, stage ") + stage + ": " + (e != hipSuccess ? hipGetErrorString(e) : "stream synchronised") +
                    "; RCCL: " + rccl_detail(comm, async));
  return CURVIS_OK;
}

int curvis_ctx_bcast_skies(curvis_ctx *ctx, void *nccl_comm, int root) {
  if (!ctx || !nccl_comm) return fail(ctx, CURVIS_E_INVALID, "null context or communicator");
  ncclComm_t comm = (ncclComm_t)nccl_comm;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rank = -1;
  ncclResult_t nrc = ncclCommUserRank(comm, &rank);
  if (nrc != ncclSuccess) return fail(ctx, CURVIS_E_RCCL, "sky broadcast, stage communicator: ncclCommUserRank: " + rccl_detail(comm, nrc));
  /* header first: {root_ok, w0, h0, w1, h1}, then the two textures.  root_ok travels with the shapes so that a
   * root without skies makes EVERY rank return CURVIS_E_NO_SKY together -- a root that returned before the
   * collective would leave its peers waiting inside ncclBroadcast for ever. */
  DeviceBuffer<uint32_t> d_hdr; /* freed on every return below */
  int rc = d_hdr.reserve(ctx, 5);
  if (rc) return rc;
  uint32_t hdr[5] = {0u, ctx->sky[0].w, ctx->sky[0].h, ctx->sky[1].w, ctx->sky[1].h};
  if (rank == root) {
    hdr[0] = (ctx->sky[0].texels && ctx->sky[1].texels) ? 1u : 0u;
    HIP_TRY(ctx, hipMemcpyAsync(d_hdr, hdr, sizeof hdr, hipMemcpyHostToDevice, ctx->stream));
  }
  nrc = ncclBroadcast(d_hdr.p, d_hdr.p, 5, ncclUint32, root, comm, ctx->stream);
  if (nrc != ncclSuccess)
    return fail(ctx, CURVIS_E_RCCL, "sky broadcast, stage header_broadcast: ncclBroadcast: " + rccl_detail(comm, nrc));
  rc = bcast_stage_sync(ctx, comm, "header_broadcast");
  if (rc != CURVIS_OK) return rc;
  const hipError_t e = hipMemcpy(hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost);
  if (e != hipSuccess)
    return fail(ctx, CURVIS_E_HIP, std::string("sky broadcast, stage header_broadcast: reading the header back: ") + hipGetErrorString(e));
  if (hdr[0] != 1u)
    return fail(ctx, CURVIS_E_NO_SKY, rank == root ? "root rank must hold both skies before the broadcast"
                                                   : "the root rank of the sky broadcast holds no skies");
  const uint32_t *shape = hdr + 1;
  for (int s = 0; s < 2; ++s) ctx->sky[s].drop_mips(); /* option "sky_mipmap": every device rebuilds its own chain; it is not broadcast */
  for (int s = 0; s < 2; ++s) {
    const uint32_t w = shape[2 * s], h = shape[2 * s + 1];
    const char *stage = s == 0 ? "texture_broadcast(+l sky)" : "texture_broadcast(-l sky)";
    if (rank != root) {
      rc = curvis_ctx_set_sky(ctx, s, nullptr, w, h);
      if (rc) return fail(ctx, rc, std::string("sky broadcast, stage ") + stage + ": allocating the receiving texture: " + ctx->err);
    }
    nrc = ncclBroadcast(ctx->sky[s].texels, ctx->sky[s].texels, (size_t)w * h * 4, ncclUint8, root, comm, ctx->stream);
    if (nrc != ncclSuccess)
      return fail(ctx, CURVIS_E_RCCL, std::string("sky broadcast, stage ") + stage + ": ncclBroadcast: " + rccl_detail(comm, nrc));
    rc = bcast_stage_sync(ctx, comm, stage); /* one synchronisation per texture: the error names the texture */
    if (rc != CURVIS_OK) return rc;
  }
  return CURVIS_OK;
}

/* How two devices of this node are connected (hipExtGetLinkTypeAndHopCount / hipDeviceGetP2PAttribute): read next to the
 * first measured sky_broadcast_gbps -- xGMI is point-to-point, 7 links x ~153 GB/s per MI355X; a pair that only has PCIe
 * between it explains a broadcast an order of magnitude slower.  link_type: HSA_AMD_LINK_INFO_TYPE_* (2 PCIe, 4 xGMI),
 * 0 with hops 0 for a == b, -1 unknown.  Every output pointer may be NULL. */
int curvis_device_link(int device_a, int device_b, int *link_type, int *hops, int *peer_access, int *performance_rank,
                       int *native_atomics) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_a < 0 || device_b < 0 || device_a >= n || device_b >= n)
    return fail(nullptr, CURVIS_E_INVALID, "curvis_device_link: no such device");
  int lt = -1, hp = -1, pa = -1, pr = -1, na = -1;
  if (device_a == device_b) {
    lt = 0, hp = 0, pa = 1;
  } else {
    uint32_t t = 0, h = 0;
    if (hipExtGetLinkTypeAndHopCount(device_a, device_b, &t, &h) == hipSuccess) lt = (int)t, hp = (int)h;
    int v = 0;
    if (hipDeviceCanAccessPeer(&v, device_a, device_b) == hipSuccess) pa = v;
    if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrPerformanceRank, device_a, device_b) == hipSuccess) pr = v;
    if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrNativeAtomicSupported, device_a, device_b) == hipSuccess) na = v;
    (void)hipGetLastError();
  }
  if (link_type) *link_type = lt;
  if (hops) *hops = hp;
  if (peer_access) *peer_access = pa;
  if (performance_rank) *performance_rank = pr;
  if (native_atomics) *native_atomics = na;
  return CURVIS_OK;
}

static_assert(sizeof(ncclUniqueId) == CURVIS_RCCL_ID_BYTES, "ncclUniqueId is 128 bytes in RCCL");

/* the ranks of these communicators sit on ONE node (frames of a video shard over the GPUs of a node): RCCL's bootstrap goes
 * over the loopback interface unless the user has chosen one -- on hosts whose first interface is slow or unroutable the
 * default choice was seen to cost 6 s to ~80 s of communicator set-up */
static void rccl_single_node_defaults() { ::setenv("NCCL_SOCKET_IFNAME", "lo", 0); }

int curvis_rccl_unique_id(uint8_t id[CURVIS_RCCL_ID_BYTES]) {
  if (!id) return fail(nullptr, CURVIS_E_INVALID, "null id");
  rccl_single_node_defaults();
  ncclUniqueId u;
  const ncclResult_t rc = ncclGetUniqueId(&u);
  if (rc != ncclSuccess) return fail(nullptr, CURVIS_E_RCCL, std::string("ncclGetUniqueId: ") + ncclGetErrorString(rc));
  std::memcpy(id, &u, sizeof u);
  return CURVIS_OK;
}

int curvis_ctx_rccl_comm_init(curvis_ctx *ctx, const uint8_t id[CURVIS_RCCL_ID_BYTES], int n_ranks, int rank,
                              void **comm_out) {
  if (!ctx || !id || !comm_out || n_ranks < 1 || rank < 0 || rank >= n_ranks)
    return fail(ctx, CURVIS_E_INVALID, "bad argument");
  *comm_out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rccl_single_node_defaults();
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  ncclComm_t comm = nullptr;
  const ncclResult_t rc = ncclCommInitRank(&comm, n_ranks, u, rank);
  if (rc != ncclSuccess)
    return fail(ctx, CURVIS_E_RCCL, "ncclCommInitRank (rank " + std::to_string(rank) + " of " + std::to_string(n_ranks) + ", device " +
                                        std::to_string(ctx->device) + "): " + rccl_detail(nullptr, rc));
  *comm_out = (void *)comm;
  return CURVIS_OK;
}

int curvis_rccl_comm_destroy(void *nccl_comm) {
  if (!nccl_comm) return CURVIS_OK;
  return ncclCommDestroy((ncclComm_t)nccl_comm) == ncclSuccess ? CURVIS_OK : CURVIS_E_RCCL;
}

int curvis_ctx_read_sky(curvis_ctx *ctx, int which, size_t offset, size_t bytes, uint8_t *out) {
  if (!ctx || !out || which < 0 || which > 1) return fail(ctx, CURVIS_E_INVALID, "bad argument");
  if (!ctx->sky[which].texels) return fail(ctx, CURVIS_E_NO_SKY, "sky not set");
  const size_t total = ctx->sky[which].bytes();
  if (offset > total || bytes > total - offset) return fail(ctx, CURVIS_E_INVALID, "range outside the texture");
  if (bytes == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(out, (const uint8_t *)ctx->sky[which].texels + offset, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

int curvis_orientation_init(const double forward[3], const double up[3], double rot[9], double inv_rot[9],
                            double up_out[3]) {
  if (!forward || !up) return CURVIS_E_INVALID;
  cvh::Orientation o;
  if (!cvh::orientation_new(cvh::Vec3{forward[0], forward[1], forward[2]}, cvh::Vec3{up[0], up[1], up[2]}, o))
    return CURVIS_E_PARALLEL;
  if (rot) std::memcpy(rot, o.rotation.m, sizeof o.rotation.m);
  if (inv_rot) std::memcpy(inv_rot, o.inverse_rotation.m, sizeof o.inverse_rotation.m);
  if (up_out) {
    up_out[0] = o.up.x;
    up_out[1] = o.up.y;
    up_out[2] = o.up.z;
  }
  return CURVIS_OK;
}

int curvis_camera_init(curvis_camera *out, const double pos[4], const double forward[3], const double up[3],
                       double focal_length, double sensor_diagonal, uint32_t res_x, uint32_t res_y) {
  if (!out || !pos || !forward || !up) return CURVIS_E_INVALID;
  if (!(focal_length > 0.0)) return CURVIS_E_INVALID;    /* src/cameras.rs:92 */
  if (!(sensor_diagonal > 0.0)) return CURVIS_E_INVALID; /* :95 */
  if (res_x == 0 || res_y == 0) return CURVIS_E_INVALID; /* :98 */
  int rc = curvis_orientation_init(forward, up, out->rot, nullptr, nullptr);
  if (rc) return rc;
  for (int i = 0; i < 4; ++i) out->pos[i] = pos[i];
  const double aspect = (double)res_x / (double)res_y; /* :107-110 */
  const double aspect2 = aspect * aspect;
  out->sensor_h = std::sqrt(sensor_diagonal * sensor_diagonal / (aspect2 + 1.0));
  out->sensor_w = aspect * out->sensor_h;
  out->focal = focal_length;
  out->res_x = res_x;
  out->res_y = res_y;
  return CURVIS_OK;
}

int curvis_metric_validate(const curvis_metric *m) {
  if (!m) return CURVIS_E_INVALID;
  switch (m->kind) {
    case CURVIS_METRIC_ELLIS:
      return (m->rho <= 0.0 || m->rho != m->rho) ? CURVIS_E_METRIC : CURVIS_OK;
    case CURVIS_METRIC_INTERSTELLAR:
      if (m->m <= 0.0 || m->a <= 0.0 || m->rho <= 0.0) return CURVIS_E_METRIC;
      if (m->m != m->m || m->a != m->a || m->rho != m->rho) return CURVIS_E_METRIC;
      return CURVIS_OK;
    case CURVIS_METRIC_FLAT:
      return CURVIS_OK;
    case CURVIS_METRIC_SCHWARZSCHILD: /* the mass in m; rho and a are ignored */
      return (m->m > 0.0) ? CURVIS_OK : CURVIS_E_METRIC; /* false for a NaN */
    default:
      return CURVIS_E_METRIC;
  }
}

int curvis_metric_functions(const curvis_metric *m, double l, double *r, double *r_squared, double *r_derivative) {
  if (!m) return CURVIS_E_INVALID;
  if (curvis_metric_validate(m) != CURVIS_OK) return CURVIS_E_METRIC;
  const cvk::MetricParams MP = make_metric(*m);
  double rr, r2, rd;
  with_kind(m->kind, [&](auto K) { cvk::metric_eval<decltype(K)::value>(MP, l, rr, r2, rd); });
  if (r) *r = rr;
  if (r_squared) *r_squared = r2;
  if (r_derivative) *r_derivative = rd;
  return CURVIS_OK;
}

int curvis_schwarzschild_u(const curvis_metric *m, double l, double *u) {
  if (!m || !u || m->kind != CURVIS_METRIC_SCHWARZSCHILD) return CURVIS_E_INVALID;
  if (curvis_metric_validate(m) != CURVIS_OK) return CURVIS_E_METRIC;
  *u = cvk::schwarzschild_u(make_metric(*m), l);
  return CURVIS_OK;
}

int curvis_ctx_set_disc_motion(curvis_ctx *ctx, int motion, double gain) {
  if (!ctx) return CURVIS_E_INVALID;
  if (motion < -1 || motion > 1) return fail(ctx, CURVIS_E_INVALID, "disc motion: must be 0 (static), 1 (prograde, +phi) or -1 (retrograde)");
  if (!std::isfinite(gain) || gain < 0.0) return fail(ctx, CURVIS_E_INVALID, "disc motion: the gain must be finite and not negative");
  ctx->disc_motion = motion, ctx->disc_gain = gain;
  return CURVIS_OK;
}

int curvis_disc_shift(const curvis_metric *m, double l_hit, double l_camera, int motion, double gain, double p_phi, double *F) {
  if (!m || !F || m->kind != CURVIS_METRIC_SCHWARZSCHILD || motion < -1 || motion > 1) return CURVIS_E_INVALID;
  if (curvis_metric_validate(m) != CURVIS_OK) return CURVIS_E_METRIC;
  *F = motion == 0 ? 1.0 : cvk::disc_shift(make_metric(*m), l_hit, l_camera, (double)motion, gain, p_phi);
  return CURVIS_OK;
}

int curvis_disc_shade(uint32_t texel, double F, uint32_t *out) {
  if (!out) return CURVIS_E_INVALID;
  *out = cvk::disc_shade(texel, F);
  return CURVIS_OK;
}

int curvis_metric_tensor(const curvis_metric *m, const double position[4], double g_cov[4], double g_contr[4]) {
  if (!m || !position) return CURVIS_E_INVALID;
  double r2;
  const int rc = curvis_metric_functions(m, position[1], nullptr, &r2, nullptr);
  if (rc != CURVIS_OK) return rc;
  const double s = cv_sin(position[2]);
  const double g[4] = {-1.0, 1.0, r2, r2 * (s * s)};
  for (int i = 0; i < 4; ++i) {
    if (g_cov) g_cov[i] = g[i];
    if (g_contr) g_contr[i] = 1.0 / g[i];
  }
  return CURVIS_OK;
}

int curvis_camera_outward_vector(const curvis_camera *camera, uint32_t px, uint32_t py, double camera_space[3],
                                 double world_space[3]) {
  if (!camera || camera->res_x == 0 || camera->res_y == 0) return CURVIS_E_INVALID;
  /* the first half of cvk::ray_init, expression for expression */
  const double h = 0.5 - ((double)py / (double)camera->res_y);
  const double w = ((double)px / (double)camera->res_x) - 0.5;
  double vx = camera->focal * 1.0;
  double vy = -camera->sensor_w * w;
  double vz = camera->sensor_h * h;
  const double n = std::sqrt(vx * vx + vy * vy + vz * vz);
  vx = vx / n;
  vy = vy / n;
  vz = vz / n;
  if (camera_space) {
    camera_space[0] = vx;
    camera_space[1] = vy;
    camera_space[2] = vz;
  }
  if (world_space) cvk::mat3_vec(camera->rot, vx, vy, vz, world_space[0], world_space[1], world_space[2]);
  return CURVIS_OK;
}

int curvis_camera_outward_vector_projected(const curvis_camera *camera, int32_t projection, uint32_t px, uint32_t py, double camera_space[3],
                                           double world_space[3]) {
  if (!camera || camera->res_x == 0 || camera->res_y == 0 || projection < 0 || projection > 2) return CURVIS_E_INVALID;
  /* the first half of cvk::ray_init, by the function it calls */
  const cvk::CameraParams C = make_camera(*camera);
  double vx, vy, vz;
  cvk::camera_pixel_vector(C, (int)projection, px, py, vx, vy, vz);
  const double n = std::sqrt(vx * vx + vy * vy + vz * vz);
  vx = vx / n;
  vy = vy / n;
  vz = vz / n;
  if (camera_space) {
    camera_space[0] = vx;
    camera_space[1] = vy;
    camera_space[2] = vz;
  }
  if (world_space) cvk::mat3_vec(C.rot, vx, vy, vz, world_space[0], world_space[1], world_space[2]);
  return CURVIS_OK;
}

int curvis_ctx_set_camera_velocities(curvis_ctx *ctx, const double *beta, uint32_t n) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!beta || n == 0) {
    ctx->cam_beta.clear();
    return CURVIS_OK;
  }
  for (uint32_t k = 0; k < n; ++k) {
    const double *b = beta + 3 * (size_t)k;
    if (!((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2] < 1.0))
      return fail(ctx, CURVIS_E_INVALID, "camera velocity: the speed of triple " + std::to_string(k) + " is not below 1 (the speed of light)");
  }
  ctx->cam_beta.assign(beta, beta + 3 * (size_t)n);
  return CURVIS_OK;
}

int curvis_camera_boost_prepare(const curvis_camera *camera, const double beta[3], double out[5]) {
  if (!camera || !beta || !out) return CURVIS_E_INVALID;
  cvk::CameraBoost K;
  if (cvk::camera_boost_prepare(camera->rot, beta, K) < 0) return CURVIS_E_INVALID;
  out[0] = K.u[0], out[1] = K.u[1], out[2] = K.u[2], out[3] = K.A, out[4] = K.B;
  return CURVIS_OK;
}

int curvis_camera_outward_vector_boosted(const curvis_camera *camera, int32_t projection, const double beta[3], uint32_t px, uint32_t py,
                                         double camera_space[3], double world_space[3]) {
  if (!camera || !beta || camera->res_x == 0 || camera->res_y == 0 || projection < 0 || projection > 2) return CURVIS_E_INVALID;
  /* the first half of cvk::ray_init, by the functions it calls */
  const cvk::CameraParams C = make_camera(*camera);
  cvk::CameraBoost K;
  if (cvk::camera_boost_prepare(C.rot, beta, K) < 0) return CURVIS_E_INVALID;
  double vx, vy, vz;
  cvk::camera_pixel_vector(C, (int)projection, px, py, vx, vy, vz);
  cvk::camera_boost(K, vx, vy, vz);
  const double n = std::sqrt(vx * vx + vy * vy + vz * vz);
  vx = vx / n;
  vy = vy / n;
  vz = vz / n;
  if (camera_space) {
    camera_space[0] = vx;
    camera_space[1] = vy;
    camera_space[2] = vz;
  }
  if (world_space) cvk::mat3_vec(C.rot, vx, vy, vz, world_space[0], world_space[1], world_space[2]);
  return CURVIS_OK;
}

int curvis_camera_path_velocity(const curvis_metric *metric, const double pos_prev[4], const double pos[4], const double pos_next[4],
                                double light_speed, double beta_out[3]) {
  if (!metric || !pos_prev || !pos || !pos_next || !beta_out) return CURVIS_E_INVALID;
  double r;
  if (const int rc = curvis_metric_functions(metric, pos[1], &r, nullptr, nullptr)) return rc;
  const double dt = pos_next[0] - pos_prev[0];
  if (dt == 0.0) {
    beta_out[0] = beta_out[1] = beta_out[2] = 0.0;
    return CURVIS_OK;
  }
  const double inv = 1.0 / (dt * light_speed);
  beta_out[0] = (pos_next[1] - pos_prev[1]) * inv;
  beta_out[1] = r * (pos_next[2] - pos_prev[2]) * inv;
  beta_out[2] = (r * cv_sin(pos[2])) * (pos_next[3] - pos_prev[3]) * inv;
  return CURVIS_OK;
}

int curvis_vector_to_direction(const curvis_metric *metric, const double position[4], const double p_cov[4],
                               double direction[3]) {
  if (!metric || !position || !p_cov || !direction) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return CURVIS_E_METRIC;
  const cvk::MetricParams MP = make_metric(*metric);
  cvk::Ray q;
  q.l = position[1];
  q.th = position[2];
  q.ph = position[3];
  q.p1 = p_cov[1];
  q.p2 = p_cov[2];
  q.p3 = p_cov[3];
  q.p3sq = q.p3 * q.p3;
  with_kind(metric->kind, [&](auto K) { cvk::ray_direction<decltype(K)::value>(MP, q, direction[0], direction[1], direction[2]); });
  return CURVIS_OK;
}

int curvis_update_relativistic_object(const curvis_metric *metric, double x[4], double p_cov[4], double delta) {
  if (!metric || !x || !p_cov) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return CURVIS_E_METRIC;
  const cvk::MetricParams MP = make_metric(*metric);
  with_kind(metric->kind, [&](auto K) { host_euler_step<decltype(K)::value>(MP, x, p_cov, delta); });
  return CURVIS_OK;
}

int curvis_step_delta(double delta, int64_t step_scale, double l, double *out) {
  static_assert(cvk::kStepScaleMax == (long long)CURVIS_STEP_SCALE_MAX, "one bound");
  return cvk::step_delta_of_scale(delta, (long long)step_scale, l, out) ? CURVIS_OK : CURVIS_E_INVALID;
}

int curvis_heun_step(const curvis_metric *metric, double x[4], double p_cov[4], double delta) {
  if (!metric || !x || !p_cov) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return CURVIS_E_METRIC;
  const cvk::MetricParams MP = make_metric(*metric);
  with_kind(metric->kind, [&](auto K) { cvk::heun_step_all<decltype(K)::value>(MP, x, p_cov, delta); });
  return CURVIS_OK;
}

int curvis_walk_ray(const curvis_metric *metric, double x[4], double p_cov[4], double delta, int64_t step_scale, int32_t integrator,
                    uint32_t max_iterations, double max_radius, uint32_t *steps, int32_t *code) {
  if (!metric || !x || !p_cov || !steps || !code || (integrator != 0 && integrator != 1)) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return CURVIS_E_METRIC;
  double probe;
  if (!cvk::step_delta_of_scale(delta, (long long)step_scale, 0.0, &probe)) return CURVIS_E_INVALID;
  if (integrator != 0 && !(delta > 0.0)) return CURVIS_E_INVALID;
  const cvk::MetricParams MP = make_metric(*metric);
  const bool adapt = step_scale != 0 || integrator != 0;
  const double kappa = step_scale != 0 ? cvk::step_kappa(delta, (long long)step_scale) : 0.0;
  *steps = max_iterations;
  *code = CURVIS_NOT_ESCAPED;
  if (max_iterations == 0) return CURVIS_OK;
  with_kind(metric->kind, [&](auto K) { /* the loop of geodesic_static, with the IEEE form of the step */
    constexpr int KIND = decltype(K)::value;
    for (uint32_t k = 1;; ++k) {
      const double dk = adapt ? cvk::step_delta(delta, kappa, x[1]) : delta;
      if (integrator) cvk::heun_step_all<KIND>(MP, x, p_cov, dk);
      else host_euler_step<KIND>(MP, x, p_cov, dk);
      if (std::fabs(x[1]) > max_radius) {
        *steps = k;
        *code = x[1] > 0.0 ? CURVIS_POSITIVE_SPACE : CURVIS_NEGATIVE_SPACE;
        break;
      }
      if (k >= max_iterations) break;
    }
  });
  return CURVIS_OK;
}

int curvis_sky_texel_index(uint32_t w, uint32_t h, const double inv_rot[9], const double v[3], uint32_t *x, uint32_t *y) {
  if (!v || !x || !y || w == 0 || h == 0) return CURVIS_E_INVALID;
  cvk::SkyParams S;
  S.texels = nullptr;
  S.w = w;
  S.h = h;
  for (int i = 0; i < 9; ++i) S.inv_rot[i] = inv_rot ? inv_rot[i] : ((i % 4 == 0) ? 1.0 : 0.0);
  unsigned tx = 0, ty = 0;
  cvk::sky_indices(S, v[0], v[1], v[2], tx, ty);
  *x = tx;
  *y = ty;
  return (tx >= w || ty >= h) ? CURVIS_E_INVALID : CURVIS_OK;
}

int curvis_sky_bilinear_taps(uint32_t w, uint32_t h, const double inv_rot[9], const double v[3], uint32_t taps[6], uint32_t raw[2]) {
  if (!v || !taps || !raw || w == 0 || h == 0) return CURVIS_E_INVALID;
  cvk::SkyParams S;
  S.texels = nullptr;
  S.w = w;
  S.h = h;
  for (int i = 0; i < 9; ++i) S.inv_rot[i] = inv_rot ? inv_rot[i] : ((i % 4 == 0) ? 1.0 : 0.0);
  if (w > kSkyFilterMaxSide || h > kSkyFilterMaxSide) { /* 256 w no longer a u32: the nearest indices, no taps */
    unsigned tx = 0, ty = 0;
    cvk::sky_indices(S, v[0], v[1], v[2], tx, ty);
    raw[0] = tx, raw[1] = ty;
    for (int i = 0; i < 6; ++i) taps[i] = 0;
    return CURVIS_E_INVALID;
  }
  cvk::SkyTaps t;
  cvk::sky_bilinear_taps(S, v[0], v[1], v[2], t);
  taps[0] = t.x0, taps[1] = t.x1, taps[2] = t.y0, taps[3] = t.y1, taps[4] = t.fx, taps[5] = t.fy;
  raw[0] = t.tx, raw[1] = t.ty;
  return t.oob ? CURVIS_E_INVALID : CURVIS_OK;
}

int curvis_sky_mip_rho(uint32_t w, const uint32_t own[2], const uint32_t horizontal[2], int32_t horizontal_ok, const uint32_t vertical[2],
                       int32_t vertical_ok, uint32_t *rho) {
  if (!own || !horizontal || !vertical || !rho || w == 0 || w > kSkyFilterMaxSide) return CURVIS_E_INVALID;
  *rho = cvk::sky_mip_rho(own[0], own[1], w << 8, horizontal[0], horizontal[1], horizontal_ok != 0, vertical[0], vertical[1], vertical_ok != 0);
  return CURVIS_OK;
}

int curvis_sky_mip_level(uint32_t rho, uint32_t levels, uint32_t *k, uint32_t *f) {
  if (!k || !f || levels == 0) return CURVIS_E_INVALID;
  unsigned kk, ff;
  cvk::sky_mip_level(rho, levels, kk, ff);
  *k = kk, *f = ff;
  return CURVIS_OK;
}

int curvis_sky_mip_taps(uint32_t w, uint32_t h, uint32_t level, uint32_t xc, uint32_t yc, uint32_t taps[6], uint32_t size[2]) {
  if (!taps || !size || w == 0 || h == 0 || w > kSkyFilterMaxSide || h > kSkyFilterMaxSide) return CURVIS_E_INVALID;
  if (level >= cvk::sky_mip_levels(w, h) || xc >= (w << 8) || yc >= (h << 8)) return CURVIS_E_INVALID;
  unsigned wk = w, hk = h;
  for (uint32_t k = 0; k < level; ++k) wk = (wk + 1u) >> 1, hk = (hk + 1u) >> 1;
  cvk::SkyTaps t;
  cvk::sky_mip_taps(xc >> level, yc >> level, wk, hk, t);
  taps[0] = t.x0, taps[1] = t.x1, taps[2] = t.y0, taps[3] = t.y1, taps[4] = t.fx, taps[5] = t.fy;
  size[0] = wk, size[1] = hk;
  return CURVIS_OK;
}

int curvis_sky_mip_mix(uint32_t ck, uint32_t ck1, uint32_t f, uint32_t *out) {
  if (!out || f > 255u) return CURVIS_E_INVALID;
  *out = cvk::sky_mip_mix(ck, ck1, f);
  return CURVIS_OK;
}

int curvis_sky_mip_pyramid(const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t level, uint8_t *out, uint32_t *wl, uint32_t *hl) {
  if (!rgba || !wl || !hl || w == 0 || h == 0 || level >= cvk::sky_mip_levels(w, h)) return CURVIS_E_INVALID;
  std::vector<unsigned> cur((size_t)w * h), next;
  std::memcpy(cur.data(), rgba, cur.size() * 4);
  unsigned wk = w, hk = h;
  for (uint32_t k = 0; k < level; ++k) {
    const unsigned wd = (wk + 1u) >> 1, hd = (hk + 1u) >> 1;
    next.assign((size_t)wd * hd, 0u);
    for (unsigned y = 0; y < hd; ++y)
      for (unsigned x = 0; x < wd; ++x) {
        const unsigned x0 = 2u * x, x1 = x0 + 1u < wk ? x0 + 1u : wk - 1u, y0 = 2u * y, y1 = y0 + 1u < hk ? y0 + 1u : hk - 1u;
        next[(size_t)y * wd + x] = cvk::sky_mip_down(cur[(size_t)y0 * wk + x0], cur[(size_t)y0 * wk + x1], cur[(size_t)y1 * wk + x0], cur[(size_t)y1 * wk + x1]);
      }
    cur.swap(next);
    wk = wd, hk = hd;
  }
  *wl = wk, *hl = hk;
  if (out) std::memcpy(out, cur.data(), cur.size() * 4);
  return CURVIS_OK;
}

int curvis_ctx_sky_mip_level(curvis_ctx *ctx, int which, uint32_t level, uint8_t *out, uint32_t *w, uint32_t *h) {
  if (!ctx) return CURVIS_E_INVALID;
  if (which < 0 || which > 1 || !w || !h) return fail(ctx, CURVIS_E_INVALID, "bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_sky_mips(ctx, which)) return rc;
  const SkyTexture &S = ctx->sky[which];
  if (level >= S.mip_levels) return fail(ctx, CURVIS_E_INVALID, "sky_mipmap: no such level");
  const cvk::SkyMipLevel &lv = S.mip_host[level];
  *w = lv.w, *h = lv.h;
  if (!out) return CURVIS_OK;
  HIP_TRY(ctx, hipMemcpyAsync(out, lv.texels, (size_t)lv.w * lv.h * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

int curvis_render_brute(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                        uint32_t max_iterations, double max_radius, double delta, uint8_t *rgb_out,
                        curvis_stats *stats) {
  return render_impl(ctx, metric, camera, 1, max_iterations, max_radius, delta, rgb_out, nullptr, stats);
}

int curvis_render_brute_rows(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                             uint32_t row_begin, uint32_t row_count, uint32_t max_iterations, double max_radius,
                             double delta, uint8_t *rgb_out, curvis_stats *stats) {
  if (row_count == 0) return fail(ctx, CURVIS_E_INVALID, "row_count must be greater than 0");
  return render_impl(ctx, metric, camera, 1, max_iterations, max_radius, delta, rgb_out, nullptr, stats, row_begin,
                     row_count);
}

int curvis_render_brute_debug(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                              uint32_t max_iterations, double max_radius, double delta, uint8_t *rgb_out,
                              curvis_ray_debug *dbg_out, curvis_stats *stats) {
  if (!dbg_out) return fail(ctx, CURVIS_E_INVALID, "dbg_out is null");
  return render_impl(ctx, metric, camera, 1, max_iterations, max_radius, delta, rgb_out, dbg_out, stats);
}

int curvis_render_brute_batch(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras,
                              uint32_t n_frames, uint32_t max_iterations, double max_radius, double delta,
                              uint8_t *rgb_out, curvis_stats *stats) {
  return render_impl(ctx, metric, cameras, n_frames, max_iterations, max_radius, delta, rgb_out, nullptr, stats);
}

/* the efficient and the direct renderer reduce every ray to an equatorial orbit: no theta, no plane to cross */
static int refuse_disc(curvis_ctx *ctx, const char *renderer) {
  if (!ctx) return CURVIS_OK; /* the call itself says so */
  ctx->last_frame_disc.clear();
  if (!ctx->disc_set) return CURVIS_OK;
  return fail(ctx, CURVIS_E_INVALID, std::string("a disc is set: ") + renderer + " reduces every ray to an equatorial orbit and cannot see it -- the brute renderer does (or remove the disc: curvis_ctx_set_disc with rgba = NULL)");
}

int curvis_render_efficient(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera,
                            uint32_t max_iterations_propagation, double max_radius, double delta, uint32_t alpha_nums,
                            uint32_t max_iterations_sampling, double sampling_convergence_threshold_1,
                            double sampling_convergence_threshold_2, uint8_t *rgb_out, curvis_stats *stats) {
  const EfficientCall call = {metric, camera, 1, max_iterations_propagation, max_radius, delta, alpha_nums, max_iterations_sampling,
                              sampling_convergence_threshold_1, sampling_convergence_threshold_2};
  if (int rc = refuse_disc(ctx, "the efficient renderer")) return rc;
  return render_efficient_impl(ctx, call, rgb_out, stats);
}

int curvis_render_efficient_batch(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras,
                                  uint32_t n_frames, uint32_t max_iterations_propagation, double max_radius,
                                  double delta, uint32_t alpha_nums, uint32_t max_iterations_sampling,
                                  double sampling_convergence_threshold_1, double sampling_convergence_threshold_2,
                                  uint8_t *rgb_out, curvis_stats *stats) {
  const EfficientCall call = {metric, cameras, n_frames, max_iterations_propagation, max_radius, delta, alpha_nums, max_iterations_sampling,
                              sampling_convergence_threshold_1, sampling_convergence_threshold_2};
  if (int rc = refuse_disc(ctx, "the efficient renderer")) return rc;
  return render_efficient_impl(ctx, call, rgb_out, stats);
}

int curvis_ctx_prefetch_efficient(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cameras, uint32_t n_frames,
                                  uint32_t max_iterations_propagation, double max_radius, double delta, uint32_t alpha_nums,
                                  uint32_t max_iterations_sampling, double sampling_convergence_threshold_1,
                                  double sampling_convergence_threshold_2) {
  const EfficientCall call = {metric, cameras, n_frames, max_iterations_propagation, max_radius, delta, alpha_nums, max_iterations_sampling,
                              sampling_convergence_threshold_1, sampling_convergence_threshold_2};
  if (ctx && ctx->disc_set) return fail(ctx, CURVIS_E_INVALID, "a disc is set: the efficient renderer, whose sampler this call runs ahead of time, cannot see it");
  return prefetch_efficient_impl(ctx, call);
}

int curvis_render_direct(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *camera, uint32_t max_iterations,
                         double max_radius, double delta, uint8_t *rgb_out, curvis_stats *stats) {
  if (int rc = refuse_disc(ctx, "the direct renderer")) return rc;
  return render_direct_impl(ctx, metric, camera, max_iterations, max_radius, delta, rgb_out, stats);
}

int curvis_ctx_sampling_info(const curvis_ctx *ctx, uint32_t frame, curvis_sampling_info *info) {
  if (!ctx || !info || frame >= ctx->last_sampling_info.size()) return CURVIS_E_INVALID;
  *info = ctx->last_sampling_info[frame];
  return CURVIS_OK;
}

int curvis_ctx_frame_stats(const curvis_ctx *ctx, uint32_t frame, curvis_stats *stats) {
  if (!ctx || !stats || frame >= ctx->last_frame_stats.size()) return CURVIS_E_INVALID;
  *stats = ctx->last_frame_stats[frame];
  return CURVIS_OK;
}

int curvis_ctx_frame_disc_hits(const curvis_ctx *ctx, uint32_t frame, uint64_t *n_disc) {
  if (!ctx || !n_disc || frame >= ctx->last_frame_stats.size()) return CURVIS_E_INVALID;
  *n_disc = frame < ctx->last_frame_disc.size() ? ctx->last_frame_disc[frame] : 0;
  return CURVIS_OK;
}

int curvis_ctx_samples(const curvis_ctx *ctx, uint32_t frame, double *alpha, double *escape_angle,
                       double *escape_space, size_t cap) {
  if (!ctx || frame >= ctx->last_samples.size()) return CURVIS_E_INVALID;
  /* device-resident sampler: the tables stayed in HBM; this frame's is fetched now (the context is the caller's to mutate: a
   * context is not thread-safe, and the const in the signature promises nothing about caches) */
  const int frc = fetch_device_samples(const_cast<curvis_ctx *>(ctx), frame);
  if (frc != CURVIS_OK) return frc;
  const auto &pts = ctx->last_samples[frame];
  if (cap < pts.size()) return CURVIS_E_INVALID;
  for (size_t i = 0; i < pts.size(); ++i) {
    if (alpha) alpha[i] = pts[i].a;
    if (escape_angle) escape_angle[i] = pts[i].e;
    if (escape_space) escape_space[i] = pts[i].s;
  }
  return CURVIS_OK;
}

int curvis_new_photon(const curvis_metric *metric, const double position[4], const double direction[3], double x[4],
                      double p_cov[4]) {
  if (!metric || !position || !direction || !x || !p_cov) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return CURVIS_E_METRIC;
  const cvk::MetricParams MP = make_metric(*metric);
  cvk::Ray q;
  with_kind(metric->kind, [&](auto K) { cvk::ray_init_dir<decltype(K)::value>(MP, position, direction[0], direction[1], direction[2], q); });
  for (int i = 0; i < 4; ++i) x[i] = position[i];
  p_cov[0] = 1.0;
  p_cov[1] = q.p1;
  p_cov[2] = q.p2;
  p_cov[3] = q.p3;
  return CURVIS_OK;
}

int curvis_photon_trajectories(curvis_ctx *ctx, const curvis_metric *metric, uint32_t n_photons, const double *x0,
                               const double *p0_cov, uint32_t iterations, double delta, double *out) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!metric || !x0 || !p0_cov || !out) return fail(ctx, CURVIS_E_INVALID, "null argument");
  if (curvis_metric_validate(metric) != CURVIS_OK) return fail(ctx, CURVIS_E_METRIC, "invalid metric parameters");
  if (n_photons == 0 || iterations == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t in_bytes = (size_t)n_photons * 4 * sizeof(double);
  const size_t out_bytes = (size_t)n_photons * iterations * 8 * sizeof(double);
  int rc = ctx->d_eff.reserve(ctx, 2 * in_bytes + out_bytes);
  if (rc) return rc;
  double *d_x = (double *)ctx->d_eff.p, *d_p = d_x + (size_t)n_photons * 4, *d_out = d_p + (size_t)n_photons * 4;
  HIP_TRY(ctx, hipMemcpyAsync(d_x, x0, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_p, p0_cov, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  TrajectoryParams P;
  P.metric = make_metric(*metric);
  P.x0 = d_x;
  P.p0 = d_p;
  P.out = d_out;
  P.n = n_photons;
  P.iterations = iterations;
  P.delta = delta;
  const unsigned blocks = (n_photons + 63u) / 64u;
  with_kind(metric->kind, [&](auto K) {
    hipLaunchKernelGGL((trajectory_kernel<decltype(K)::value>), dim3(blocks), dim3(64), 0, ctx->stream, P);
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

int curvis_compute_escape_angles(curvis_ctx *ctx, const curvis_metric *metric, double l, const double *alphas,
                                 uint32_t n, double delta, uint32_t max_iterations, double max_radius,
                                 double *angle, int32_t *space, uint32_t *steps) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!metric || !alphas || !angle || !space) return fail(ctx, CURVIS_E_INVALID, "null argument");
  if (curvis_metric_validate(metric) != CURVIS_OK) return fail(ctx, CURVIS_E_METRIC, "invalid metric parameters");
  if (std::fabs(l) > max_radius)
    return fail(ctx, CURVIS_E_CAMERA_OUTSIDE,
                "Photon already beyond the maximum radius. Cannot evaluate escape. (src/systems.rs:122-124)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const cvk::MetricParams MP = make_metric(*metric);
  std::vector<double> a(alphas, alphas + n), ls(n, l), ang, spc;
  std::vector<uint32_t> st;
  std::vector<int> status;
  int rc = eval_escape_batch(ctx, metric, MP, a, ls, max_iterations, max_radius, delta, ang, spc, st, status, nullptr);
  if (rc) return rc;
  bool panic = false;
  for (uint32_t i = 0; i < n; ++i) {
    angle[i] = ang[i];
    space[i] = status[i] == cvk::ESC_PANIC ? 0 : status[i];
    if (steps) steps[i] = st[i];
    if (status[i] == cvk::ESC_PANIC) panic = true;
  }
  if (panic) return fail(ctx, CURVIS_E_PARALLEL, "v1 and v2 must not be parallel (src/algebra.rs:95-97) for at least one sample");
  return CURVIS_OK;
}

int curvis_image_load(const char *path, uint8_t **rgba_out, uint32_t *w, uint32_t *h) {
  if (!path || !rgba_out || !w || !h) return fail(nullptr, CURVIS_E_INVALID, "null argument");
  *rgba_out = nullptr;
  pngio::Image img;
  std::string err;
  if (!jpegio::load_image(path, img, err)) return fail(nullptr, CURVIS_E_IO, std::string(path) + ": " + err);
  uint8_t *buf = (uint8_t *)std::malloc(img.rgba.size() ? img.rgba.size() : 1);
  if (!buf) return fail(nullptr, CURVIS_E_IO, "out of memory");
  std::memcpy(buf, img.rgba.data(), img.rgba.size());
  *rgba_out = buf;
  *w = img.w;
  *h = img.h;
  return CURVIS_OK;
}

void curvis_image_free(uint8_t *rgba) { std::free(rgba); }

int curvis_image_save_rgb8(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h) {
  if (!path || !rgb || w == 0 || h == 0) return fail(nullptr, CURVIS_E_INVALID, "null argument or empty image");
  std::string err;
  if (!pngio::save_rgb8(path, rgb, w, h, err)) return fail(nullptr, CURVIS_E_IO, err);
  return CURVIS_OK;
}

int curvis_image_save_rgb8_level(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h, int level) {
  if (!path || !rgb || w == 0 || h == 0) return fail(nullptr, CURVIS_E_INVALID, "null argument or empty image");
  if (level < -1 || level > 9) return fail(nullptr, CURVIS_E_INVALID, "level must be -1 (fast writer) or 0..9 (zlib)");
  std::string err;
  if (!pngio::save_rgb8(path, rgb, w, h, err, level)) return fail(nullptr, CURVIS_E_IO, err);
  return CURVIS_OK;
}

int curvis_ctx_deflate_frames(curvis_ctx *ctx, uint32_t res_x, uint32_t res_y, uint32_t n_frames, uint8_t *zlib_out, size_t out_cap,
                              size_t *offsets, double *kernel_ms) {
  return deflate_frames_impl(ctx, res_x, res_y, n_frames, zlib_out, out_cap, offsets, kernel_ms);
}

int curvis_ctx_deflate_frames_crc(curvis_ctx *ctx, uint32_t res_x, uint32_t res_y, uint32_t n_frames, uint8_t *zlib_out, size_t out_cap,
                                  size_t *offsets, double *kernel_ms, uint32_t *idat_crc, int *crc_valid) {
  if (!idat_crc || !crc_valid) return fail(ctx, CURVIS_E_INVALID, "null idat_crc / crc_valid");
  return deflate_frames_impl(ctx, res_x, res_y, n_frames, zlib_out, out_cap, offsets, kernel_ms, idat_crc, crc_valid);
}

int curvis_image_save_zlib_rgb8_crc(const char *path, const uint8_t *zlib_stream, size_t len, uint32_t w, uint32_t h, uint32_t idat_crc) {
  if (!path || !zlib_stream || len < 6 || w == 0 || h == 0) return fail(nullptr, CURVIS_E_INVALID, "null argument or empty stream");
  std::string err;
  if (!pngio::save_zlib_stream_rgb8(path, zlib_stream, len, w, h, err, nullptr, &idat_crc)) return fail(nullptr, CURVIS_E_IO, err);
  return CURVIS_OK;
}

int curvis_image_save_zlib_rgb8(const char *path, const uint8_t *zlib_stream, size_t len, uint32_t w, uint32_t h) {
  if (!path || !zlib_stream || len < 6 || w == 0 || h == 0) return fail(nullptr, CURVIS_E_INVALID, "null argument or empty stream");
  std::string err;
  if (!pngio::save_zlib_stream_rgb8(path, zlib_stream, len, w, h, err)) return fail(nullptr, CURVIS_E_IO, err);
  return CURVIS_OK;
}

int curvis_host_alloc(size_t bytes, void **out) {
  if (!out || bytes == 0) return fail(nullptr, CURVIS_E_INVALID, "curvis_host_alloc: null pointer or zero bytes");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable); /* usable from every device's context */
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(nullptr, CURVIS_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  return CURVIS_OK;
}
void curvis_host_free(void *p) {
  PinnedBuffer<unsigned char> adopted; /* freed as it leaves the scope */
  adopted.p = (unsigned char *)p;
}

int curvis_ctx_framebuffer(curvis_ctx *ctx, void **dev_ptr, size_t *bytes) {
  if (!ctx) return CURVIS_E_INVALID;
  if (dev_ptr) *dev_ptr = ctx->d_fb.p;
  if (bytes) *bytes = ctx->fb_bytes;
  return CURVIS_OK;
}

int curvis_ctx_download(curvis_ctx *ctx, uint8_t *rgb_out, size_t bytes) {
  if (!ctx || !rgb_out) return CURVIS_E_INVALID;
  if (bytes > ctx->fb_bytes) return fail(ctx, CURVIS_E_INVALID, "download larger than the last frame");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(rgb_out, ctx->d_fb, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

/* the other direction: RGB8 frames from host memory into the context's framebuffer (it grows as needed), so that frames
 * made elsewhere -- a host that composites, a test with chosen contents -- can go through curvis_ctx_deflate_frames */
int curvis_ctx_upload(curvis_ctx *ctx, const uint8_t *rgb, size_t bytes) {
  if (!ctx || !rgb || bytes == 0) return fail(ctx, CURVIS_E_INVALID, "bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = fb_begin_write(ctx, bytes);
  if (rc) return rc;
  ctx->fb_bytes = bytes;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_fb, rgb, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

int curvis_ctx_synchronize(curvis_ctx *ctx) {
  if (!ctx) return CURVIS_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CURVIS_OK;
}

/* option "async_download": the frames of the last render call that was given `rgb_out` are in host memory on return */
int curvis_ctx_download_wait(curvis_ctx *ctx) {
  if (!ctx) return CURVIS_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return download_wait(ctx);
}

} /* extern "C" */

namespace {

/* ---- options: ONE table of keys.  curvis_ctx_set_option and curvis_ctx_get_option walk it; a key without a writer is a statistic
 * (read-only: setting it is refused like a key that does not exist), a key without a reader is a test hook that is consumed by
 * the code it arms.  Values travel as int64_t and are stored through the type named here. */
struct OptionEntry {
  const char *key;
  int64_t (*read)(const curvis_ctx *);  /* or null */
  int (*write)(curvis_ctx *, int64_t);  /* or null */
};
#define OPT_READ(expr) [](const curvis_ctx *c) -> int64_t { return (int64_t)(expr); }
#define OPT_WRITE(field, type) [](curvis_ctx *c, int64_t v) -> int { c->field = (type)v; return CURVIS_OK; }
#define OPT_RW(field, type) {#field, OPT_READ(c->field), OPT_WRITE(field, type)}
#define OPT_RO(key, expr) {key, OPT_READ(expr), nullptr}

/* "async_download" / "async_streams" (fb_download in render_host.h, deflate_frames_impl in png_host.h): switching one off waits for
 * what is in flight first, and keeps the flag if that wait fails */
int drain_before_switching_off(curvis_ctx *c, int64_t v) {
  if (v) return CURVIS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return download_wait(c);
}

const OptionEntry kOptions[] = {
    OPT_RW(variant, int),
    OPT_RW(refill_threshold, int),
    OPT_RW(blocks_per_cu, int),
    OPT_RW(block_threads, int),
    OPT_RW(relay_segment, int),
    OPT_RW(relay_max_hops, int),
    OPT_RW(relay_max_parks, int),
    OPT_RW(relay_recheck_every, int),
    {"async_download", OPT_READ(c->async_download),
     [](curvis_ctx *c, int64_t v) -> int {
       if (int rc = drain_before_switching_off(c, v)) return rc;
       c->async_download = v ? 1 : 0;
       return CURVIS_OK;
     }},
    {"async_streams", OPT_READ(c->async_streams),
     [](curvis_ctx *c, int64_t v) -> int {
       if (int rc = drain_before_switching_off(c, v)) return rc;
       c->async_streams = v ? 1 : 0;
       return CURVIS_OK;
     }},
    OPT_RW(relay_max_frames, int),
    OPT_RW(relay_min_blocks, long long),
    OPT_RW(relay_verify, int),
    {"relay_auto_verify", OPT_READ(c->relay_auto_verify),
     [](curvis_ctx *c, int64_t v) -> int {
       c->relay_auto_verify = (int)v;
       c->relay_verified.clear(); /* switching it (back) on checks every shape afresh */
       return CURVIS_OK;
     }},
    {"relay_test_corrupt", nullptr, OPT_WRITE(relay_test_corrupt, int)}, /* consumed by launch_relay */
    OPT_RW(relay_disabled, int),
    {"relay_test_fault", nullptr, OPT_WRITE(relay_test_fault, int)},     /* consumed by render_chunk's re-launch loop */
    OPT_RW(fast_math, int),
    OPT_RW(fuse_shade, int),
    {"supersample", OPT_READ(c->supersample),
     [](curvis_ctx *c, int64_t v) -> int { /* divisors of 8: a pixel's rays then sit in one wave's 8x8 tile (resolve_store) */
       if (v != 1 && v != 2 && v != 4 && v != 8) return fail(c, CURVIS_E_INVALID, "supersample must be 1, 2, 4 or 8");
       c->supersample = (int)v;
       return CURVIS_OK;
     }},
    {"sky_filter", OPT_READ(c->sky_filter),
     [](curvis_ctx *c, int64_t v) -> int {
       if (v != 0 && v != 1) return fail(c, CURVIS_E_INVALID, "sky_filter must be 0 (nearest) or 1 (bilinear)");
       c->sky_filter = (int)v;
       return CURVIS_OK;
     }},
    {"sky_mipmap", OPT_READ(c->sky_mipmap), /* always settable, in either order with "sky_filter": a render call checks the pair */
     [](curvis_ctx *c, int64_t v) -> int {
       if (v != 0 && v != 1) return fail(c, CURVIS_E_INVALID, "sky_mipmap must be 0 (off) or 1 (on)");
       c->sky_mipmap = (int)v;
       return CURVIS_OK;
     }},
    {"projection", OPT_READ(c->projection),
     [](curvis_ctx *c, int64_t v) -> int {
       if (v < 0 || v > 2) return fail(c, CURVIS_E_INVALID, "projection must be 0 (perspective), 1 (equirectangular) or 2 (fisheye)");
       c->projection = (int)v;
       return CURVIS_OK;
     }},
    {"step_scale", OPT_READ(c->step_scale),
     [](curvis_ctx *c, int64_t v) -> int {
       if (v < 0 || v > (int64_t)CURVIS_STEP_SCALE_MAX) return fail(c, CURVIS_E_INVALID, "step_scale must be 0 (off) or L0 x 256 in 1 .. 2^20");
       c->step_scale = v;
       return CURVIS_OK;
     }},
    {"integrator", OPT_READ(c->integrator),
     [](curvis_ctx *c, int64_t v) -> int {
       if (v != 0 && v != 1) return fail(c, CURVIS_E_INVALID, "integrator must be 0 (Euler) or 1 (Heun)");
       c->integrator = (int)v;
       return CURVIS_OK;
     }},
    OPT_RW(pixel_tiled, int), /* measurement switch: 1 = the efficient renderer enumerates pixels by 8x8 tiles whatever the other options say */
    OPT_RW(device_sampler, int),
    {"device_sampler_min_frames", OPT_READ(c->device_sampler_min_frames),
     [](curvis_ctx *c, int64_t v) -> int {
       c->device_sampler_min_frames = v < 1 ? 1 : (int)v;
       return CURVIS_OK;
     }},
    OPT_RW(sampling_speculation, int),
    OPT_RW(sampling_speculation_first, int),
    OPT_RW(max_store_bytes, size_t),
    /* statistics */
    OPT_RO("relay_mismatches", c->relay_mismatches),
    OPT_RO("relay_verified_shapes", c->relay_verified.size()),
    OPT_RO("relay_checks", c->relay_checks),
    OPT_RO("last_png_stream_bytes", c->last_png_stream_bytes),
    OPT_RO("streams_pending", c->streams_pending ? 1 : 0),
    OPT_RO("downloads_overlapped", c->downloads_overlapped),
    OPT_RO("download_pending", c->dl_pending ? 1 : 0),
    OPT_RO("relay_fallbacks", c->relay_fallbacks),
    OPT_RO("last_frames", c->last_frame_stats.size()),
    OPT_RO("last_relay_launches", c->last_relay_launches),
    OPT_RO("last_relay_parks", c->last_relay_parks),
    OPT_RO("last_relay_waiters", c->last_relay_waiters),
    OPT_RO("last_sampler_path", c->last_sampler_path),
    OPT_RO("last_pixel_tiled", c->last_pixel_tiled),
    OPT_RO("last_sky_mip_build_us", c->last_sky_mip_build_us),
    OPT_RO("last_sky_copy_us", c->last_sky_copy_us),
    OPT_RO("last_sampling_chains", c->last_sampling_chains),
    OPT_RO("last_sampling_prefetched", c->last_sampling_prefetched),
    OPT_RO("prefetches", c->prefetches),
    OPT_RO("prefetch_hits", c->prefetch_hits),
    OPT_RO("last_sampling_launches", c->last_sampling_launches),
    OPT_RO("last_sampling_evaluated", c->last_sampling_evaluated),
};
#undef OPT_RO
#undef OPT_RW
#undef OPT_WRITE
#undef OPT_READ

const OptionEntry *find_option(const char *key) {
  for (const OptionEntry &o : kOptions)
    if (std::strcmp(o.key, key) == 0) return &o;
  return nullptr;
}

}  // namespace

extern "C" {

int curvis_ctx_set_option(curvis_ctx *ctx, const char *key, int64_t value) {
  if (!ctx || !key) return CURVIS_E_INVALID;
  const OptionEntry *o = find_option(key);
  if (!o || !o->write) return fail(ctx, CURVIS_E_INVALID, std::string("unknown option ") + key);
  return o->write(ctx, value);
}

int curvis_ctx_get_option(const curvis_ctx *ctx, const char *key, int64_t *value) {
  if (!ctx || !key || !value) return CURVIS_E_INVALID;
  const OptionEntry *o = find_option(key);
  if (!o || !o->read) return CURVIS_E_INVALID;
  *value = o->read(ctx);
  return CURVIS_OK;
}

int curvis_selftest_math(curvis_ctx *ctx, int op, const double *a, const double *b, double *out, size_t n) {
  if (!ctx || !a || !out) return CURVIS_E_INVALID;
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<double> da, db, dout;
  if (int rc = da.reserve(ctx, n)) return rc;
  if (int rc = dout.reserve(ctx, n)) return rc;
  HIP_TRY(ctx, hipMemcpy(da, a, n * sizeof(double), hipMemcpyHostToDevice));
  if (b) {
    if (int rc = db.reserve(ctx, n)) return rc;
    HIP_TRY(ctx, hipMemcpy(db, b, n * sizeof(double), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(selftest_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, da.p, db.p, dout.p, n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
  return CURVIS_OK;
}

int curvis_selftest_math3(curvis_ctx *ctx, int op, const double *a, const double *b, const double *c, double *out, size_t n) {
  if (!ctx || !a || !out) return CURVIS_E_INVALID;
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const double *in[3] = {a, b, c};
  DeviceBuffer<double> dev[4]; /* a, b, c (each may be absent), out */
  for (int k = 0; k < 4; ++k) {
    if (k < 3 && !in[k]) continue;
    if (int rc = dev[k].reserve(ctx, n)) return rc;
    if (k < 3) HIP_TRY(ctx, hipMemcpy(dev[k], in[k], n * sizeof(double), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(selftest_math3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, dev[0].p, dev[1].p, dev[2].p,
                     dev[3].p, n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, dev[3], n * sizeof(double), hipMemcpyDeviceToHost));
  return CURVIS_OK;
}

int curvis_selftest_fast_step(curvis_ctx *ctx, const curvis_metric *metric, double delta, double max_radius, const double *states,
                              size_t n, double *out) {
  if (!ctx || !metric || !states || !out) return CURVIS_E_INVALID;
  if (curvis_metric_validate(metric) != CURVIS_OK) return fail(ctx, CURVIS_E_INVALID, "curvis_selftest_fast_step: invalid metric");
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const cvk::MetricParams MP = make_metric(*metric);
  DeviceBuffer<double> din, dout;
  if (int rc = din.reserve(ctx, n * 5)) return rc;
  if (int rc = dout.reserve(ctx, n * CURVIS_FAST_STEP_RECORD)) return rc;
  HIP_TRY(ctx, hipMemcpy(din, states, n * 5 * sizeof(double), hipMemcpyHostToDevice));
  with_kind(metric->kind, [&](auto K) {
    hipLaunchKernelGGL((selftest_fast_step_kernel<decltype(K)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, MP,
                       delta, max_radius, din.p, n, dout.p);
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, dout, n * CURVIS_FAST_STEP_RECORD * sizeof(double), hipMemcpyDeviceToHost));
  return CURVIS_OK;
}

int curvis_selftest_sky_indices(curvis_ctx *ctx, uint32_t w, uint32_t h, const double inv_rot[9], const double *dirs, size_t n,
                                uint32_t *out) {
  if (!ctx || !inv_rot || !dirs || !out) return CURVIS_E_INVALID;
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  cvk::SkyParams S;
  S.texels = nullptr; /* sky_indices does not read texels */
  S.w = w;
  S.h = h;
  for (int i = 0; i < 9; ++i) S.inv_rot[i] = inv_rot[i];
  /* y_pi, y_two_pi from where efficient_pixel_kernel's P.recips come from (they do not depend on the resolution: a cached one is kept) */
  const curvis_ctx::PixRecips &cached = ctx->pix_recips;
  cvk::PixelRecips R;
  if (int rc = ensure_pixel_recips(ctx, cached.valid ? cached.res_x : 1.0, cached.valid ? cached.res_y : 1.0, R)) return rc;
  DeviceBuffer<double> din;
  DeviceBuffer<unsigned> dout;
  if (int rc = din.reserve(ctx, n * 3)) return rc;
  if (int rc = dout.reserve(ctx, n * 4)) return rc;
  HIP_TRY(ctx, hipMemcpy(din, dirs, n * 3 * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(selftest_sky_indices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, S, R, din.p, n, dout.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, dout, n * 4 * sizeof(unsigned), hipMemcpyDeviceToHost));
  return CURVIS_OK;
}

int curvis_selftest_sky_bilinear(curvis_ctx *ctx, uint32_t w, uint32_t h, const double inv_rot[9], const uint8_t *rgba, const double *dirs,
                                 size_t n, uint32_t *out_taps, uint8_t *out_rgb) {
  if (!ctx || !inv_rot || !rgba || !dirs || !out_taps || !out_rgb || w == 0 || h == 0) return CURVIS_E_INVALID;
  if (w > kSkyFilterMaxSide || h > kSkyFilterMaxSide) return fail(ctx, CURVIS_E_INVALID, "sky_filter: a sky of more than 2^23 texels per side");
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const curvis_ctx::PixRecips &cached = ctx->pix_recips;
  cvk::PixelRecips R; /* as curvis_selftest_sky_indices */
  if (int rc = ensure_pixel_recips(ctx, cached.valid ? cached.res_x : 1.0, cached.valid ? cached.res_y : 1.0, R)) return rc;
  DeviceBuffer<double> din;
  DeviceBuffer<unsigned> dsky, dtaps;
  DeviceBuffer<unsigned char> drgb;
  const size_t texels = (size_t)w * h;
  if (int rc = dsky.reserve(ctx, texels)) return rc;
  if (int rc = din.reserve(ctx, n * 3)) return rc;
  if (int rc = dtaps.reserve(ctx, n * 12)) return rc;
  if (int rc = drgb.reserve(ctx, n * 6)) return rc;
  HIP_TRY(ctx, hipMemcpy(dsky, rgba, texels * 4, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(din, dirs, n * 3 * sizeof(double), hipMemcpyHostToDevice));
  cvk::SkyParams S;
  S.texels = dsky.p;
  S.w = w;
  S.h = h;
  for (int i = 0; i < 9; ++i) S.inv_rot[i] = inv_rot[i];
  hipLaunchKernelGGL(selftest_sky_bilinear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, S, R, din.p, n, dtaps.p, drgb.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out_taps, dtaps, n * 12 * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(out_rgb, drgb, n * 6, hipMemcpyDeviceToHost));
  return CURVIS_OK;
}

int curvis_selftest_sky_mip(curvis_ctx *ctx, uint32_t w, uint32_t h, const uint8_t *rgba, const uint32_t *triples, size_t n, uint8_t *out_rgb) {
  if (!ctx || !rgba || !triples || !out_rgb || w == 0 || h == 0) return CURVIS_E_INVALID;
  if (w > kSkyFilterMaxSide || h > kSkyFilterMaxSide) return fail(ctx, CURVIS_E_INVALID, "sky_mipmap: a sky of more than 2^23 texels per side");
  if (n == 0) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<unsigned> dsky, dchain, din, dout;
  DeviceBuffer<cvk::SkyMipLevel> dtab;
  std::vector<cvk::SkyMipLevel> tab;
  unsigned L = 0;
  const size_t texels = (size_t)w * h;
  if (int rc = dsky.reserve(ctx, texels)) return rc;
  if (int rc = din.reserve(ctx, n * 3)) return rc;
  if (int rc = dout.reserve(ctx, n)) return rc;
  HIP_TRY(ctx, hipMemcpy(dsky, rgba, texels * 4, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(din, triples, n * 3 * sizeof(unsigned), hipMemcpyHostToDevice));
  if (int rc = build_sky_mips(ctx, dsky.p, w, h, dchain, dtab, tab, L)) return rc;
  hipLaunchKernelGGL(selftest_sky_mip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dtab.p, L, din.p, n, dout.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<unsigned> packed(n);
  HIP_TRY(ctx, hipMemcpy(packed.data(), dout, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i)
    out_rgb[3 * i] = (uint8_t)(packed[i] & 0xFF), out_rgb[3 * i + 1] = (uint8_t)((packed[i] >> 8) & 0xFF), out_rgb[3 * i + 2] = (uint8_t)((packed[i] >> 16) & 0xFF);
  return CURVIS_OK;
}

} /* extern "C" */
