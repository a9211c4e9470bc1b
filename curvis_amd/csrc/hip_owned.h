/* hip_owned.h -- the owners of the library's HIP resources: device and page-locked buffers, events, streams, a sky texture.
 * Move-only (or fixed in place), freed by their destructors; failures are reported through fail / HIP_TRY like everything else.
 * A buffer that lives for one call is a local DeviceBuffer: it is freed on every return path, the error returns included.
 * Part of the ONE translation unit curvis_hip.hip (included there, nowhere else). */
#pragma once

struct curvis_ctx;

namespace {

int fail(curvis_ctx *ctx, int code, const std::string &msg); /* render_host.h: needs the context's members */

#define HIP_TRY(ctx, call)                                                                         \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(ctx, CURVIS_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
  } while (0)

/* `cap` elements of T at `p`, in HBM or (PINNED) in page-locked host memory */
template <typename T, bool PINNED>
struct HipBuffer {
  T *p = nullptr;
  size_t cap = 0;
  HipBuffer() = default;
  HipBuffer(HipBuffer &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  HipBuffer &operator=(HipBuffer &&o) noexcept { /* (std::swap of two buffers is three of these) */
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~HipBuffer() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
  }
  /* room for `need` elements; grows only, and then to need + headroom.  The contents are NOT kept: the old block is freed first
   * (pointer and capacity zeroed before the allocation that can fail), so that the two never add up. */
  int reserve(curvis_ctx *ctx, size_t need, size_t headroom = 0) {
    if (need <= cap) return CURVIS_OK;
    if (p) HIP_TRY(ctx, PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
    const size_t n = need + headroom;
    HIP_TRY(ctx, PINNED ? hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, n * sizeof(T)));
    cap = n;
    return CURVIS_OK;
  }
  operator T *() const { return p; }
};
template <typename T>
using DeviceBuffer = HipBuffer<T, false>;
template <typename T>
using PinnedBuffer = HipBuffer<T, true>;

/* created on first use, with the flags of that use */
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  int ensure(curvis_ctx *ctx, unsigned flags = hipEventDefault) {
    if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, flags));
    return CURVIS_OK;
  }
  operator hipEvent_t() const { return e; }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  int ensure(curvis_ctx *ctx, unsigned flags = hipStreamNonBlocking) {
    if (!s) HIP_TRY(ctx, hipStreamCreateWithFlags(&s, flags));
    return CURVIS_OK;
  }
  operator hipStream_t() const { return s; }
};

/* a background image: w x h RGBA8 texels in HBM, the library's own copy or (curvis_ctx_set_sky_device, copy = 0) the caller's */
struct SkyTexture {
  void *texels = nullptr;
  bool owned = false;
  unsigned w = 0, h = 0;
  /* option "sky_mipmap": levels 1 .. mip_levels - 1 of the mip chain in one allocation, and the level table the kernels index
   * (entry 0 points at `texels`); built by the first render call with the option on (render_host.h ensure_sky_mips), dropped with the
   * texels.  mip_levels = 0: not built -- nothing is allocated for a context that never sets the option */
  DeviceBuffer<unsigned> mip_texels;
  DeviceBuffer<cvk::SkyMipLevel> mip_table;
  std::vector<cvk::SkyMipLevel> mip_host; /* the table's host copy */
  unsigned mip_levels = 0;
  void drop_mips() {
    mip_texels = DeviceBuffer<unsigned>();
    mip_table = DeviceBuffer<cvk::SkyMipLevel>();
    mip_host.clear();
    mip_levels = 0;
  }
  SkyTexture() = default;
  SkyTexture(const SkyTexture &) = delete;
  SkyTexture &operator=(const SkyTexture &) = delete;
  ~SkyTexture() {
    if (texels && owned) (void)hipFree(texels);
  }
  size_t bytes() const { return (size_t)w * h * 4; }
  /* drop the texels (free them if they are ours) and take a new shape; nothing is allocated yet */
  int reset(curvis_ctx *ctx, unsigned w_, unsigned h_) {
    drop_mips(); /* first: a failed hipFree below must not leave a chain of the old texels attached */
    if (texels && owned) HIP_TRY(ctx, hipFree(texels));
    texels = nullptr;
    owned = false;
    w = w_;
    h = h_;
    return CURVIS_OK;
  }
  int allocate(curvis_ctx *ctx) { /* after reset */
    HIP_TRY(ctx, hipMalloc(&texels, bytes()));
    owned = true;
    return CURVIS_OK;
  }
  void borrow(const void *dev_rgba) { /* after reset; the caller keeps it alive */
    texels = const_cast<void *>(dev_rgba);
    owned = false;
  }
};

}  // namespace
